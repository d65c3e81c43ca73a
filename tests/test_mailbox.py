"""One-sided mailbox gossip (bcfl.parallel.mailbox): the CPU analogue (shared-memory inboxes,
gloo for the one start-up handle exchange) of the hipIpc transport. Properties: posts need no
matching receive, torn snapshots are rejected, tampered payloads fail the Merkle commitment and are
recorded in the ledger, and a slow or EXITED peer never stalls the others."""
import json
import os
import time

import numpy as np
import pytest
import torch

from dist_utils import run_world


def _cfg(out, **kw):
    from bcfl.config import FLConfig
    base = dict(mode="serverless", model="tiny-bert", dataset="tiny", num_clients=2, num_rounds=3,
                train_samples=48, test_samples=16, global_test_samples=32, batch_size=16, lr=1e-3,
                out_dir=out, partition="label_shards", reference_prints=False, save_every=0,
                device="cpu", backend="gloo", async_gossip=True, gossip_transport="mailbox")
    base.update(kw)
    return FLConfig(**base)


def _transport_worker(rank, world):
    from bcfl.parallel import dist as D
    from bcfl.parallel.mailbox import MailboxTransport, Snapshot
    D.init_runtime("cpu", "gloo")
    peer = 1 - rank
    tr = MailboxTransport(1000, torch.float32, torch.device("cpu"), listen=[peer],
                          send_plan=[(rank, peer)])
    try:
        D.barrier()
        x = torch.arange(1000, dtype=torch.float32) + 1000 * rank
        tr.post(rank, x, Snapshot(1, 0, 8, 4000, bytes(range(32))))
        D.barrier()  # only so the test knows the post landed; the protocol never waits
        out = {peer: torch.zeros(1000)}
        got = tr.fetch({peer: 0}, out)
        again = tr.fetch({peer: 1}, out)  # nothing newer than version 1
        D.barrier()
        # a half-written version 3 (begin without end) lands in slot 1, over version 1: the
        # reader finds no complete snapshot and keeps what it holds
        tr.backend.hdr_store(tr.outbox[rank][0][1].hdr, 1, [3], 0)
        D.barrier()
        torn_view = tr.fetch({peer: 1}, out)
        return {"data": out[peer].clone(), "version": torch.tensor(got[peer].version),
                "root_ok": torch.tensor(got[peer].root == bytes(range(32))),
                "again": torch.tensor(len(again)), "half": torch.tensor(len(torn_view))}
    finally:
        D.barrier()
        tr.close()


def test_mailbox_transport_post_fetch(tmp_path):
    res = run_world(_transport_worker, 2, str(tmp_path))
    assert torch.equal(res[0]["data"], torch.arange(1000, dtype=torch.float32) + 1000)
    assert torch.equal(res[1]["data"], torch.arange(1000, dtype=torch.float32))
    for r in res:
        assert int(r["version"]) == 1 and bool(r["root_ok"])
        assert int(r["again"]) == 0 and int(r["half"]) == 0


def _fed_worker(rank, world, out, kw, stop_after=None, test_barrier=False):
    from bcfl.fl import Federation
    from bcfl.parallel import dist as D
    fed = Federation(_cfg(out, **kw), verbose=False)
    times = []
    for r in range(fed.cfg.num_rounds):
        if stop_after is not None and rank == 1 and r == stop_after:
            return {"exited": torch.tensor(1)}  # this rank leaves for good, mid-run
        t0 = time.perf_counter()
        fed.run_round(r)
        times.append(time.perf_counter() - t0)
        if test_barrier:
            # test-only: make round r's posts visible before round r+1 fetches, so the assertion
            # on accepted updates does not depend on process scheduling (the protocol never waits)
            D.barrier()
    fed.finish(audit=stop_after is None)
    blocks = fed.ledger.blocks() if fed.ledger is not None else []
    return {"master": fed.flat.master.clone(), "times": torch.tensor(times),
            "dead": torch.tensor(sorted(fed.gossip.dead), dtype=torch.int64),
            "rejects": torch.tensor(sum(b["kind"] == "verify" and b["verdict"] == "reject"
                                        for b in blocks)),
            "accepts": torch.tensor(sum(b["kind"] == "verify" and b["verdict"] == "accept"
                                        for b in blocks)),
            "acc": torch.tensor([h["global_acc"] for h in fed.history]),
            "audit": torch.tensor(-1 if fed.ledger_audit is None else fed.ledger_audit["mismatched"])}


def test_mailbox_federation_async_runs(tmp_path):
    res = run_world(_fed_worker, 2, str(tmp_path / "d"), str(tmp_path / "d"), {}, None, True)
    for r in res:
        assert torch.isfinite(r["master"]).all()
        assert int(r["accepts"]) >= 1 and int(r["rejects"]) == 0
        assert int(r["audit"]) == 0  # every accepted update matches its sender's commitment
    assert os.path.exists(tmp_path / "d" / "ledger.jsonl")
    assert os.path.exists(tmp_path / "d" / "ledger.rank1.jsonl")


def test_mailbox_sync_equals_single_process(tmp_path):
    """Sync mailbox + fp32 wire: every round mixes the fresh snapshots, exactly like one process
    hosting both clients."""
    from bcfl.fl import Federation
    from bcfl.parallel import dist as D
    kw = {"async_gossip": False, "wire_dtype": "fp32"}
    res = run_world(_fed_worker, 2, str(tmp_path / "d"), str(tmp_path / "d"), kw)
    D.set_runtime_for_tests(None)
    nt = torch.get_num_threads()
    torch.set_num_threads(2)
    try:
        fed = Federation(_cfg(str(tmp_path / "s"), **kw), verbose=False)
        fed.run()
    finally:
        torch.set_num_threads(nt)
        D.set_runtime_for_tests(None)
    assert torch.equal(res[0]["master"], res[1]["master"])
    assert torch.equal(res[0]["master"], fed.flat.master)


def test_mailbox_tamper_rejected_and_logged(tmp_path):
    # test barrier: round r's posts land before round r + 1 fetches (on a loaded CPU rank 1 could
    # otherwise finish all three rounds before rank 0's first post and accept nothing)
    res = run_world(_fed_worker, 2, str(tmp_path / "d"), str(tmp_path / "d"),
                    {"inject_tamper": [1], "num_rounds": 3}, None, True)
    # rank 0 rejects every (corrupted) update of client 1 — once per version, not once per poll
    # (a rejected version is remembered and never re-fetched); rank 1 accepts client 0's
    assert 1 <= int(res[0]["rejects"]) <= 3 and int(res[0]["accepts"]) == 0
    assert int(res[1]["rejects"]) == 0 and int(res[1]["accepts"]) >= 1
    assert 1 in res[0]["dead"].tolist()  # never a good snapshot -> aged out of the mix
    rows = [l for l in open(tmp_path / "d" / "ledger.jsonl") if '"verify"' in l]
    assert rows and all('"reject"' in l and "merkle root mismatch" in l for l in rows)


def test_mailbox_slow_peer_does_not_stall(tmp_path):
    # client 1 (rank 1) sleeps 5 s per round; rank 0 keeps its own pace (unbounded staleness:
    # with the default bound a 5 s/round peer holds the fast rank back by design, see
    # test_mailbox_bounded_lead_holds_fast_rank_back)
    res = run_world(_fed_worker, 2, str(tmp_path / "d"), str(tmp_path / "d"),
                    {"inject_slow": {1: 5000.0}, "num_rounds": 3, "gossip_max_lead": 0})
    assert float(res[1]["times"].min()) >= 5.0
    # the first round includes setup (mailbox mapping, first exchange) and is slow on a loaded
    # CPU; every later round of rank 0 runs at its own pace, and its whole run ends well before
    # the sleeping peer's
    assert float(res[0]["times"][1:].max()) < 4.0
    assert float(res[0]["times"].sum()) < float(res[1]["times"].sum()) - 5.0


def test_mailbox_exited_peer_does_not_stall(tmp_path):
    # rank 1 leaves after round 1; rank 0 completes every round and ages client 1 out
    res = run_world(_fed_worker, 2, str(tmp_path / "d"), str(tmp_path / "d"),
                    {"num_rounds": 6, "liveness_timeout": 1}, 1)
    assert int(res[1]["exited"]) == 1
    assert len(res[0]["times"]) == 6
    assert res[0]["dead"].tolist() == [1]


def _fallback_worker(rank, world, out, how="open"):
    from bcfl.fl import Federation
    from bcfl.parallel import mailbox as mb
    if rank == 1 and how == "open":  # this rank cannot map its peers' inboxes
        def bad_open(self, handle, nbytes, owner_device=-1):
            raise OSError("simulated hipIpcOpenMemHandle failure")
        mb.ShmBackend.open = bad_open
    if rank == 1 and how == "peer":  # no xGMI / P2P path from this rank's device to its peers'
        mb.ShmBackend.peer_ok = lambda self, owner_device: False
    fed = Federation(_cfg(out), verbose=False)
    for r in range(fed.cfg.num_rounds):
        fed.run_round(r)
    fed.finish(audit=False)
    return {"transport_rccl": torch.tensor(int(fed.transport == "rccl")),
            "collective_free": torch.tensor(int(fed.collective_free)),
            "finite": torch.tensor(int(torch.isfinite(fed.flat.master).all()))}


@pytest.mark.parametrize("how", ["open", "peer"])
def test_mailbox_failure_on_one_rank_falls_back_to_rccl_everywhere(tmp_path, how):
    """A mapping failure on ONE rank — the IPC open itself, or no peer access between the two
    devices (hipDeviceCanAccessPeer = 0, checked before mapping) — is agreed collectively: every
    rank gets MailboxUnavailable and the federation continues on the lock-step RCCL (here gloo)
    engine instead of hanging or failing inside a later copy."""
    res = run_world(_fallback_worker, 2, str(tmp_path), str(tmp_path / "fb"), how)
    for r in res:
        assert int(r["transport_rccl"]) == 1 and int(r["collective_free"]) == 0
        assert int(r["finite"]) == 1


def _learn_worker(rank, world, out, kw):
    from bcfl.config import get_preset
    from bcfl.fl import Federation
    kw = dict(kw)
    torch.set_num_threads(kw.pop("threads", 2))
    # the preset's recipe (warm-up, then a constant rate, as the bench runs it); only the tiny
    # model's learning rate and the run's shape are the test's own
    base = dict(model="tiny-bert", num_clients=4, num_rounds=16, mode="serverless", lr=6e-4,
                max_seq_len=64, train_samples=256, global_test_samples=200,
                eval_local=False, save_every=0, ledger=False, device="cpu",
                reference_prints=False, out_dir=out, backend="gloo", gossip_transport="mailbox")
    base.update(kw)
    fed = Federation(get_preset("baseline3_learnable", **base), verbose=False)
    t0 = time.perf_counter()
    fed.run()
    h = fed.history
    return {"fa": fed.federation_accuracy(), "same_round": fed.same_round_mix,
            "exchange": fed.drift.exchange, "delta": fed.gossip.exchange == "delta",
            "acc": torch.tensor([x["global_acc"] for x in h]),
            "stale_max": torch.tensor(max(float(x.get("stale_max") or 0.0) for x in h)),
            "wait": torch.tensor(sum(float(x.get("wait_s") or 0.0) for x in h)),
            "elapsed": torch.tensor(time.perf_counter() - t0)}


def _check_async_learning(res, last=3, final=None):
    # accuracies travel as float32 tensors (0.9 arrives as 0.89999998): thresholds carry 1e-6
    for r in res:
        assert not r["same_round"] and r["exchange"] and r["delta"]
        assert float(r["wait"]) == 0.0                    # nothing ever waited on a peer
        assert float(r["acc"][-last:].max()) >= 0.9 - 1e-6, r["acc"].tolist()
        if final is not None:
            assert float(r["fa"]["accuracy"]) >= final - 1e-6, (r["fa"], r["acc"].tolist())
    assert max(float(r["stale_max"]) for r in res) >= 1.0   # the mixes really were stale


def test_mailbox_async_two_ranks_slow_peer_learn_label_shards(tmp_path):
    """(gossip_apply="arrival": the round-4 mode, kept for unbounded staleness) VERDICT r3 #1: label-sharded clients (one class each) on 2 ranks over the one-sided
    mailboxes, one rank slowed every round: the async gossip never waits (stale snapshots, up to
    several rounds behind, are mixed as they are) and still learns — each client's cumulative
    update is applied once (delta exchange) and its SCAFFOLD control variate travels in the same
    post (stale-exact c_hat). The round-3 alternative (state mixing of stale snapshots, mix-derived
    c') stayed near the majority rate (0.50 on MI355X, profiles/multirank_learning_r3.json).

    28 rounds: nothing paces the two ranks here, so the round at which the slowed rank's accuracy
    leaves 0.5 moves with the load on the CPU (measured: round 15-16 on an idle 8-core machine,
    >= 0.9 from round 19-20; round 19, >= 0.9 from round 22, with six busy processes beside the
    test). With 20 rounds the last three sat on that edge (0.67 / 0.76 / 0.88 in one run)."""
    res = run_world(_learn_worker, 2, str(tmp_path / "d"), str(tmp_path / "d"),
                    {"inject_slow": {1: 200.0}, "liveness_timeout": 6, "gossip_max_lead": 0,
                     "num_rounds": 28, "gossip_apply": "arrival"})
    _check_async_learning(res)


def test_mailbox_async_two_ranks_slow_peer_default_protocol(tmp_path):
    """The default protocol (round-complete application, bounded staleness 1) with one rank slowed
    every round: the fast rank is held within one round of the slow one (lead waits, bounded), every
    model holds complete rounds, and the label-sharded federation learns."""
    res = run_world(_learn_worker, 2, str(tmp_path / "d"), str(tmp_path / "d"),
                    {"inject_slow": {1: 200.0}, "num_rounds": 20})
    for r in res:
        assert not r["same_round"] and r["exchange"] and r["delta"]
        assert float(r["acc"][-3:].max()) >= 0.9 - 1e-6, r["acc"].tolist()
        assert float(r["fa"]["accuracy"]) >= 0.9 - 1e-6, r["fa"]


@pytest.mark.slow
def test_mailbox_async_four_ranks_learn_label_shards(tmp_path):
    """One client per rank (every neighbour remote: every application is of posts that crossed
    the transport) with the DEFAULT protocol: round-complete application, bounded staleness 1,
    round-tagged corrections. (Unbounded staleness, gossip_max_lead = 0, is not a supported
    learning regime for one client per rank: ranks run at their own pace and a round completes
    whenever its last post lands; round 5 measured 0.83-0.96 final accuracy over 5 runs.)"""
    res = run_world(_learn_worker, 4, str(tmp_path / "d"), str(tmp_path / "d"),
                    {"num_rounds": 24})
    for r in res:
        assert not r["same_round"] and r["exchange"] and r["delta"]
        assert float(r["acc"][-3:].max()) >= 0.9 - 1e-6, r["acc"].tolist()
        assert float(r["fa"]["accuracy"]) >= 0.9 - 1e-6, r["fa"]


@pytest.mark.slow
def test_mailbox_async_eight_ranks_default_protocol_learn_label_shards(tmp_path):
    """8 ranks (one client each, the 8-GPU layout) on 8 CPU cores — time-sliced, so
    posts land with jittery lags — with the UNMODIFIED default asynchronous protocol (delta
    exchange, round-complete application, exchanged control variates damped to 0.75, fresh AdamW
    per round, bounded staleness 1): no knob is overridden but the tiny model's learning rate and
    the run length."""
    res = run_world(_learn_worker, 8, str(tmp_path / "d"), str(tmp_path / "d"),
                    {"num_clients": 8, "num_rounds": 30})
    for r in res:
        assert not r["same_round"] and r["exchange"] and r["delta"]
        assert float(r["acc"][-3:].max()) >= 0.9 - 1e-6, r["acc"].tolist()
        assert float(r["fa"]["accuracy"]) >= 0.9 - 1e-6, r["fa"]
        # the bound holds fast ranks back a little, never stalls (relative: the suite may share
        # the 8 cores with other tests)
        assert float(r["wait"]) < 0.5 * float(r["elapsed"]), (float(r["wait"]), float(r["elapsed"]))


def test_mailbox_self_delay_runs_and_resumes_state(tmp_path):
    """gossip_self_delay = on (opt-in): a rank's own updates enter its models one round late;
    the federation still runs its async rounds and the pending updates are part of the gossip
    resume state."""
    res = run_world(_self_delay_worker, 2, str(tmp_path / "d"), str(tmp_path / "d"), {})
    for r in res:
        assert bool(r["pend_in_state"])
        assert torch.isfinite(r["acc"]).all()


def _self_delay_worker(rank, world, out, kw):
    from bcfl.config import get_preset
    from bcfl.fl import Federation
    torch.set_num_threads(2)
    fed = Federation(get_preset("baseline3_learnable", model="tiny-bert", num_clients=4, num_rounds=4,
                                mode="serverless", max_seq_len=64, train_samples=64,
                                global_test_samples=64, eval_local=False, save_every=0,
                                ledger=False, device="cpu", reference_prints=False, out_dir=out,
                                backend="gloo", gossip_transport="mailbox",
                                gossip_self_delay="on"), verbose=False)
    fed.run()
    return {"pend_in_state": torch.tensor("pend" in fed.gossip.state_dict()),
            "acc": torch.tensor([x["global_acc"] for x in fed.history])}


def test_mailbox_bounded_lead_holds_fast_rank_back(tmp_path):
    """gossip_max_lead = 1: with one rank slowed by 1.2 s per round the fast rank waits at round
    starts (lead waits > 0) instead of running away, so the staleness it mixes stays within the
    bound (+1 for the round in flight); unbounded it would drift several rounds ahead. (The delay
    must exceed a round's own time on a loaded CPU: at 400 ms the fast rank stayed under the
    2-round lead that triggers a wait in one full-suite run.)"""
    res = run_world(_learn_worker, 2, str(tmp_path / "d"), str(tmp_path / "d"),
                    {"inject_slow": {1: 1200.0}, "liveness_timeout": 6, "gossip_max_lead": 1,
                     "num_rounds": 8})
    assert float(res[0]["wait"]) > 0.0          # the fast rank was held back
    assert max(float(r["stale_max"]) for r in res) <= 3.0


def _byz_worker(rank, world, out, kw):
    from bcfl.fl import Federation
    fed = Federation(_cfg(out, **kw), verbose=False)
    fed.run()
    g = fed.gossip
    judged = [tuple(x) for h in fed.history for x in h.get("verdict_rounds", [])]
    blocks = [b for b in fed.ledger.blocks() if b["kind"] == "verdict"]
    return {"judged": judged,
            "ledger_rejects": sorted({(json.loads(b["payload"])["src_round"], b["client"])
                                      for b in blocks if b["verdict"] != "accept"}),
            "delta": torch.tensor(int(g.exchange == "delta")),
            "arrival": torch.tensor(int(g.apply_on_arrival)),
            "models": torch.stack([fed.client_master[c] for c in fed.local_clients]),
            "finite": torch.tensor(int(torch.isfinite(fed.flat.master).all()))}


def test_mailbox_delta_exchange_anomaly_filter_rejects_byzantine(tmp_path):
    """the update anomaly filter runs INSIDE the asynchronous round-complete
    protocol, with mid-round application ON (2 ranks x 2 clients, modified Z + PageRank). Each
    receiver judges a complete round's updates (sketch + norm of S_j^T - S_j^applied, measured on
    what it is about to apply) before applying any of them, so the client whose update is scaled
    50x is rejected in EVERY round, by every rank, with no collective and no previous-round
    verdicts, and its update never enters any model — its own included: every client model on
    both ranks ends on the same honest consensus."""
    res = run_world(_byz_worker, 2, str(tmp_path / "d"), str(tmp_path / "d"),
                    {"num_clients": 4, "num_rounds": 4, "anomaly_filter": "both",
                     "inject_byzantine": {1: 50.0}})
    for r in res:
        assert int(r["delta"]) == 1 and int(r["arrival"]) == 1 and int(r["finite"]) == 1
        assert [t for t, _ in r["judged"]] == [0, 1, 2, 3], r["judged"]
        assert all(list(rej) == [1] for _, rej in r["judged"]), r["judged"]
        assert r["ledger_rejects"] == [(t, 1) for t in range(4)]
    models = torch.cat([r["models"] for r in res])
    for m in models[1:]:
        torch.testing.assert_close(m, models[0], atol=1e-5, rtol=0)
