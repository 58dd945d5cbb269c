"""Direct placement of the policy keys without a GPU: the selftest's host
restatement of the direct lookup against brute force and its known answers
of pol_slot_direct against pol_direct.py's, what each case of pol_direct.py
claims about its own keys, the placement of the C2 policy table, and how many
C2 headers leave policy_resolve's first probe undecided under each
placement."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import lookup_edges as E
import oracle as O
import pol_direct as PD
from cilium_amd import _lib as L
from cilium_amd import synth as S
from cilium_amd.datapath import host_only

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_selftest_direct_placement():
    csrc = os.path.join(ROOT, "cilium_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-s", "selftest"], check=True)
    r = subprocess.run([os.path.join(csrc, "build", "selftest"), "poldirect"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    rows = dict(re.findall(r"^poldirect (\S+) .*: (\w+), max d .* -> ok$", r.stdout, flags=re.M))
    assert rows == {"random": "placed", "piled-small": "placed", "piled-home": "placed",
                    "equal-pre": "linear", "crowded": "linear"}, r.stdout[-2000:]
    kats = re.findall(r"^pd pol_slot_direct (\w+) (\w+) (\w+) (\w+)$", r.stdout, flags=re.M)
    assert len(kats) == 8 * 6 * 5
    for pre, d, mask, want in kats:
        assert int(PD.pol_slot_direct(int(pre, 16), int(d, 16), int(mask, 16))) == int(want, 16)
    # d = 0 is the linear layout's home slot; the step is odd and comes from
    # the high half of pre
    assert all(int(w, 16) == int(p, 16) & int(m, 16) for p, d, m, w in kats if d == "0")
    assert int(PD.pol_slot_direct(0x00070007, 1, 0xFFFF)) == 0x0007 + 0x0007
    assert int(PD.pol_slot_direct(0x00060007, 1, 0xFFFF)) == 0x0007 + 0x0007


@pytest.mark.parametrize("nkeys", [2, 3])
def test_smallest_tables_claim(nkeys):
    cl = PD.smallest(nkeys).claims
    dm, mask = cl["dm"], cl["mask"]
    assert mask == (7 if nkeys == 2 else 15) and dm["words"] == 64
    assert len(dm["buckets"]) == 1 and len(dm["buckets"][cl["bucket"]]) == nkeys
    assert cl["d"] >= 1 and cl["wraps"]
    for i in cl["wraps"]:   # the displaced slot lies below the home slot
        assert dm["where"][E.EP0][(i, PD.HI80)] < int(E.pol_key_pre(i, PD.HI80)) & mask
    homes = [int(E.pol_key_pre(i, PD.HI80)) & mask for i in cl["keys"][:2]]
    assert homes[0] == homes[1]
    assert len(set(dm["where"][E.EP0].values())) == nkeys


def test_shared_home_claim():
    for d in ("ingress", "egress"):
        cl = PD.shared_home(d).claims
        dm = cl["dm"]
        pa, pc = (int(E.pol_key_pre(i, PD.HI80)) for i in (cl["a"], cl["c"]))
        assert pa & 63 == pc & 63 and cl["d"] >= 1
        assert {k[1] for k in dm["buckets"][cl["bucket"]]} >= {cl["a"], cl["c"]}
        w = dm["where"][E.EP0]
        assert w[(cl["a"], PD.HI80)] != w[(cl["c"], PD.HI80)]
        # the linear layout walks for one of them
        lin = dm["linear"][E.EP0]
        assert sorted(len(E.pol_walk(dm["linear"], E.EP0, i, PD.HI80)[0])
                      for i in (cl["a"], cl["c"]))[1] >= 2
        assert lin["mask"] == 63


def test_shared_bucket_claim():
    cl = PD.shared_bucket().claims
    dm = cl["dm"]
    tabs = {k[0] for k in dm["buckets"][cl["bucket"]]}
    assert tabs == {E.EP0, E.EP0 + 1} and cl["d"] >= 1
    keys = {(k[0], k[1]) for k in dm["buckets"][cl["bucket"]]}
    assert {(E.EP0, cl["a"]), (E.EP0, cl["c"]), (E.EP0 + 1, cl["b"])} <= keys
    for lxc in tabs:   # every key where its table's one probe looks
        for (lo, hi), s in dm["where"][lxc].items():
            assert PD.first_probe(dm, lxc, lo, hi) == (s, dm["slots"][lxc][s])


def test_absent_l4_claim():
    cl = PD.absent_l4().claims
    dm = cl["dm"]
    for i, hi in ((cl["id_a"], PD.HI80), (cl["id_w"], PD.HI8080), (cl["id_n"], PD.HI80)):
        assert (i, hi) not in dm["where"][E.EP0]
        assert E.pol_maybe(dm["linear"], dm["bloom"], E.EP0, i, hi)
        s, e = PD.first_probe(dm, E.EP0, i, hi)
        assert e is not None and e[:2] != (i, hi)
    assert (cl["id_a"], 0) in dm["where"][E.EP0]
    assert (0, PD.HI8080) in dm["where"][E.EP0]
    assert not E.pol_maybe(dm["linear"], dm["bloom"], E.EP0, cl["id_n"], 0)
    assert not E.pol_maybe(dm["linear"], dm["bloom"], E.EP0, 0, PD.HI80)
    # the oracle: L3 behind -> pass, wildcard behind -> its proxy port,
    # nothing -> DROP_POLICY; fragments see the L3 key only
    c = PD.absent_l4()
    _, ver, _ = O.Oracle(c.tables).classify(c.headers, 0, 0, nthreads=4)
    sel = lambda i, p, f: (cl["ident"] == i) & (cl["dport"] == p) & (cl["frag"] == f)
    assert (ver[sel(cl["id_a"], 80, False)] == 0).all()
    assert (ver[sel(cl["id_a"], 80, True)] == 0).all()
    assert (ver[sel(cl["id_w"], 8080, False)] == int(S.htons(16000))).all()
    assert (ver[sel(cl["id_w"], 8080, True)] == E.DROP_POLICY).all()
    assert (ver[sel(cl["id_n"], 80, False)] == E.DROP_POLICY).all()
    assert (ver[sel(cl["id_n"], 80, True)] == E.DROP_POLICY).all()


def test_equal_pre_claim():
    c = PD.equal_pre()
    (lo, hi), (lo2, hi2) = c.claims["keys"]
    assert int(E.pol_key_pre(lo, hi)) == int(E.pol_key_pre(lo2, hi2))
    assert hi2 >> 24 == 0 and (hi2 >> 16) & 0xFF in (PD.TCP, PD.UDP)
    assert PD.direct_model(c.tables.policy) is None
    _, ver, _ = O.Oracle(c.tables).classify(c.headers, 0, 0, nthreads=4)
    assert {int(S.htons(11001)), int(S.htons(11002))} <= set(np.unique(ver).tolist())


def test_option_values():
    dp = host_only()
    try:
        for v in (L.POL_PLACEMENT_AUTO, L.POL_PLACEMENT_LINEAR, L.POL_PLACEMENT_DIRECT):
            dp.set_option(L.OPT_POL_PLACEMENT, v)
        for v in (-1, 3):
            with pytest.raises(OSError):
                dp.set_option(L.OPT_POL_PLACEMENT, v)
        with pytest.raises(OSError):   # no epoch yet
            dp.pol_placement()
    finally:
        dp.close()


# ------------------------------------------------------------- the C2 tables
@functools.lru_cache(None)
def c2():
    t = S.config_c2_bench(2)
    return t, PD.direct_model(t.policy)


def test_c2_table_places():
    """Measured: every bucket placed, largest d 7, 73 % of the words that
    hold a key at d 0 (7047 of 8192); the engine reports the same largest d
    for the C2 epoch."""
    t, dm = c2()
    assert dm is not None, "a bucket of the C2 table found no displacement"
    nkeys = sum(len(p) for p in t.policy.values())
    assert sum(len(w) for w in dm["where"].values()) == nkeys
    d = np.array(list(dm["disp"].values()))
    print(f"C2: {nkeys} keys, {len(d)} of {dm['words']} buckets hold a key, largest d "
          f"{dm['max_d']}, {np.mean(d == 0):.3f} at d 0")
    assert dm["max_d"] <= PD.POL_DISP_MAX
    for lxc, w in dm["where"].items():
        for (lo, hi), s in list(w.items())[::97]:
            assert PD.first_probe(dm, lxc, lo, hi) == (s, dm["slots"][lxc][s])


def test_c2_walker_share():
    """The share of 200k C2 headers (FULL mode, the oracle's identities) that
    enter policy_resolve_walk.  Measured: 0.4847 reach the policy stage,
    0.1479 probe the table; 0.0185 walk under linear probing, 0.0020 under
    the direct placement (what is left: a present key behind an absent one
    the filter passed, and real fall-through)."""
    t, _ = c2()
    h = S.headers_c2(t, 200_000)
    act, ver, ident = O.Oracle(t).classify(h, 3, 0, nthreads=8)
    la = S.local_v4_addrs(t)
    lxc = sorted(t.policy)[0]
    ep = t.endpoints[t.endpoints["lxc_id"] == lxc]
    dst = ep["addr"][:, :4].copy().view("<u4").ravel()
    assert len(t.policy) == 1 and len(dst) == 1 and dst[0] in la
    l4 = np.isin(h.proto, [PD.TCP, PD.UDP])
    reach = (h.daddr == dst[0]) & (ver != E.DROP_PREFILTER) & (l4 | (h.proto == 1))
    dport = np.where(l4, h.dport, 0)
    frag = (h.flags & S.HF_FRAG) != 0
    share = {}
    for direct in (False, True):
        probed, walks = PD.first_probe_decides(t.policy, lxc, ident[reach], dport[reach],
                                               h.proto[reach], frag[reach], direct)
        share[direct] = walks.sum() / len(h)
        print(f"{'direct' if direct else 'linear'}: reach {reach.mean():.4f}, probe "
              f"{probed.sum() / len(h):.4f}, walk {share[direct]:.4f}")
    assert 0.012 < share[False] < 0.026     # about 1.9 % under linear probing
    assert share[True] < share[False] / 2
