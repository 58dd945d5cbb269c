"""The service step's packet-order pass on the GPU at its structural edges
(svcorder.hip k_svo_mark / k_svo_replay, the override words' consumers
lb.hip k_lb4_egress and classify6.hip lb6_egress, the apply's k_cta_lb /
k_cta_svc): svc_edges.py's constructed streams — the smallest shapes, runs
across a block edge of the sorted list, keys of equal fingerprint, keys of one
home slot, chains of re-selections, headers the gates keep out, a denied
first header, stale words and workspace growth, the NAT64 hop batch's second
pass — through cfc_classify and cfc_ct_apply, once without and once with
event words, against the oracle's packet order with no header excused:
action, verdict, identity, CT byte, packet output, event words and monitor
records, the full CT dump, ct_apply_host == 0, and cfc_stats.svc_ordered's
increase equal to the builder's number exactly.  test_svc_edges.py checks on
the CPU that the streams hold what they claim.  Run on an MI355X:
pytest -m gpu."""
import numpy as np
import pytest

import oracle as O
import svc_edges as E
from cilium_amd.datapath import Datapath, pack
from cilium_amd.loader import ct_rows, load_tables

pytestmark = pytest.mark.gpu
FAMILIES = [4, 6]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    return torch


@pytest.fixture(scope="module")
def envs():
    """the tables and their histories, built once"""
    return {f: E.env(f) for f in FAMILIES}


def run_engine(torch, t, batches, notify):
    """test_gpu_lb._run over one batch after another on one datapath"""
    dp = Datapath(0)
    load_tables(dp, t)
    res = []
    for h in batches:
        b = pack(h, "cuda:0")
        before = dp.stats()["svc_ordered"]
        out = dp.classify(b, E.EGRESS, E.EP, want_ct=True, want_pkt=True, want_notify=notify)
        dp.ct_apply(b, out, E.EGRESS, E.EP)
        torch.cuda.synchronize()
        r = dict(act=out.action.cpu().numpy().astype(np.int32),
                 ver=out.verdict.cpu().numpy(),
                 ide=out.identity.cpu().numpy().view(np.uint32),
                 ct=out.ct.cpu().numpy(),
                 pkt=out.pkt.cpu().numpy().view(np.uint32))
        if notify:
            rec, idx, total = dp.monitor_events(b, out, E.EGRESS, E.EP)
            r["nt"] = out.notify.cpu().numpy().view(np.uint32)
            r["rec"] = np.ascontiguousarray(rec.cpu().numpy()).view(np.uint8).reshape(-1)
            r["idx"] = idx.cpu().numpy().astype(np.uint64)
        r["svc"] = dp.stats()["svc_ordered"] - before
        res.append(r)
    dp.counters_sync()
    rows = ct_rows(dp, dp.ct_fds)
    st = dp.stats()
    dp.close()
    return res, rows, st


def run_oracle(t, batches):
    o = O.Oracle(t)
    res = []
    for h in batches:
        act, ver, ide, ct, nt, pkt = o.classify(h, E.EGRESS, E.EP, want_ct=True,
                                                want_notify=True, want_pkt=True,
                                                apply_ct=True)
        rec, idx = o.events(h, E.EGRESS, E.EP, ver, ide, nt)
        res.append(dict(act=act, ver=ver, ide=ide, ct=ct, nt=nt, pkt=pkt, idx=idx,
                        rec=np.ascontiguousarray(rec).view(np.uint8).reshape(-1)))
    return res, o.ct_dump()


def _bad(g, w):
    """the rows at which two outputs differ"""
    assert g.shape == w.shape, (g.shape, w.shape)
    if g.size == 0:   # (a batch without events)
        return np.zeros(0, np.int64)
    return np.flatnonzero((g != w).reshape(len(g), -1).any(1))


def check_case(torch, c):
    want, want_rows = run_oracle(c.t, c.batches)
    for notify in (False, True):
        got, rows, st = run_engine(torch, c.t, c.batches, notify)
        for k, (g, w, h, n_svc) in enumerate(zip(got, want, c.batches, c.svc_ordered)):
            for f in ("act", "ver", "ide", "ct", "pkt") + (("nt", "idx") if notify else ()):
                bad = _bad(g[f], w[f])
                assert len(bad) == 0, f"batch {k} notify {notify} {f}: {len(bad)} differ, " \
                    f"first {bad[:6]} {g[f][bad[:6]]} vs {w[f][bad[:6]]}"
            if notify:
                np.testing.assert_array_equal(g["rec"], w["rec"])
            print("batch", k, "svc_ordered", g["svc"], "expected", n_svc)
            assert g["svc"] == n_svc, (k, notify, g["svc"], n_svc)
        np.testing.assert_array_equal(rows, want_rows)
        assert st["ct_apply_host"] == 0 and st["ct_apply_device"] == len(c.batches), st


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n", E.SIZES)
def test_one_flow(torch, envs, family, n):
    """n headers of one new flow, own hashes: n - 1 words (m == n at every
    size; n == 1: the list of one entry)"""
    c = E.one_flow(family, n)
    assert c.svc_ordered == [n - 1]
    check_case(torch, c)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n", E.SIZES)
def test_distinct(torch, envs, family, n):
    """n new flows of one header: every header listed, every run of length
    one, no word"""
    c = E.distinct(family, n)
    assert c.svc_ordered == [0]
    check_case(torch, c)


@pytest.mark.parametrize("family", FAMILIES)
def test_one_flow_without_hash_array(torch, envs, family):
    """hash == NULL: the pass takes the engine's flow hash, one value for the
    whole flow, and still hands on 256 words"""
    c = E.one_flow(family, 257, hashed=False)
    assert c.svc_ordered == [256]
    check_case(torch, c)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", list(E.STREAMS))
def test_stream(torch, envs, family, name):
    check_case(torch, E.stream(family, name))


def test_reslave_loopback_entry(torch, envs):
    """the re-slaved entry carries lb_loopback: the words carry SVO_LOOP"""
    check_case(torch, E.reslave(4, "loop"))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", ["collide2", "reslave_ii"])
def test_stream_in_three_chunks(torch, envs, family, name):
    """a key's headers on both sides of a cut: the later chunk finds the
    entry the earlier one's apply wrote, stable"""
    one = E.stream(family, name)
    c = E.chunked(one, 3)
    assert len(c.batches) == 3 and sum(c.svc_ordered) < one.plan.svc_ordered
    assert c.svc_ordered[0] > 0
    check_case(torch, c)


@pytest.mark.parametrize("family", FAMILIES)
def test_stale_words_and_growth(torch, envs, family):
    """one datapath: one_flow(513); the same flow, stable now, under other
    hashes; other stable flows and one listed header (a word left at any
    index would redirect that header); one_flow(2049), the workspaces grow;
    the second and third shapes again"""
    c = E.stale_and_growth(family)
    assert c.svc_ordered == [512, 0, 0, 2048, 0, 0]
    check_case(torch, c)


@pytest.mark.parametrize("m", [1, 257])
def test_nat64_hop_batch(torch, m):
    """m headers of one new flow to a v4-mapped VIP among 3 m plain IPv6
    headers: the hop batch runs the pass over its own rows (m - 1 words; a
    fresh datapath's total is the call's increase)"""
    from test_gpu_ctorder import check, run_both
    t, h, at = E.nat64_hops(m)
    g, want = run_both(torch, t, h, E.EGRESS, E.EP, clock=1003, chunks=1)
    check(g, want)
    assert g["stats"]["nat_hops"] == m, g["stats"]
    assert g["stats"]["svc_ordered"] == m - 1, g["stats"]
    assert g["stats"]["ct_apply_host"] == 0, g["stats"]
