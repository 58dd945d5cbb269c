"""The streams of test_gpu_self_edges.py (self_edges.py) hold what they claim
— checked on the CPU with the oracle alone: the Python restatement of the cut
rule against the host self-test's known answers (`selftest kat selfcut`), the
rule's sufficiency over every ordered pair of header kinds (each pair whose
packet-order result differs from its batch-start result is cut), the
expected segment count of every stream the GPU tests run, and a header that
differs on each side of every boundary the structural streams name.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import self_edges as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = [4, 6]


def test_cut_rule_restatement_matches_selfcut_hpp():
    """selftest prints a fixed pseudo-random row list per family and the cuts
    self_cut_rule gives; cut_rule gives the same"""
    csrc = os.path.join(ROOT, "cilium_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-s", "selftest"], check=True)
    r = subprocess.run([os.path.join(csrc, "build", "selftest"), "kat", "selfcut"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    fams = []
    for line in r.stdout.splitlines():
        w = line.split()
        if w[:2] == ["selfcut", "family"]:
            fams.append(dict(v6=bool(int(w[2])), n_own=int(w[3]), rows=[], cuts=[]))
        elif w[:2] == ["selfcut", "row"]:
            fams[-1]["rows"].append(tuple(int(x) for x in w[2:6]))
        elif w[:2] == ["selfcut", "cut"]:
            fams[-1]["cuts"].append(int(w[2]))
    assert [f["v6"] for f in fams] == [False, True]
    for f in fams:
        assert len(f["rows"]) >= 300
        # the list is about something: cuts, uncut rows, both address classes,
        # noise above the masked bytes
        assert 50 < len(f["cuts"]) < len(f["rows"]) - 50
        assert any(r[3] >= f["n_own"] for r in f["rows"]) and any(r[2] >> 8 for r in f["rows"])
        assert E.cut_rule(f["rows"], f["n_own"], f["v6"]) == f["cuts"]


def test_selftest_keeps_its_selfcut_cases():
    """the ten hand-written cases still run and pass"""
    exe = os.path.join(ROOT, "cilium_amd", "csrc", "build", "selftest")
    subprocess.run(["make", "-C", os.path.dirname(os.path.dirname(exe)), "-s", "selftest"],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("selfcut ")]
    assert len(lines) == 10 and all(" ok " in l for l in lines), lines


def test_catalogue_shape():
    for family in FAMILIES:
        ks = E.kinds(family)
        assert 22 <= len(ks) <= 28 and len({k[0] for k in ks}) == len(ks)
        e = E.env(family)
        own, lo = E.address_set(e.t, E.EP, family)
        assert len(own) == 1 and len(lo) == (5 if family == 4 else 4)
        for name, dst, *_ in ks:
            h = E.headers(family, [(E.kind(family, name), 1234)])
            rows, _ = E.listed_rows(e.t, h)
            assert (len(rows) == 1) == (dst not in E.NEVER_LISTED), name
            if rows:
                assert (rows[0][3] >= 1) == (dst != "own"), name


def _differ(a, b, ct=False):
    """header indices where two (action, verdict, identity, ct) views differ"""
    d = (a[0] != b[0]) | (a[1] != b[1]) | (a[2] != b[2])
    if ct:
        d |= a[3] != b[3]
    return np.flatnonzero(d)


def _views(family, blocks):
    """every block from fresh CT state, in packet order and as one batch
    looked up at its start -> per block the header indices whose action,
    verdict or identity differ, and those with the CT byte counted too"""
    t = E.env(family).t
    seq, bat = O.Oracle(t), O.Oracle(t)
    out = []
    for k, b in enumerate(blocks):
        for o in (seq, bat):
            o.set_clock(E.clock_of(k))
            o.ct_gc(time=E.clock_of(k))
        assert len(seq.ct_dump()) == 0 and len(bat.ct_dump()) == 0
        s = seq.classify(b.h, E.EGRESS, E.EP, want_ct=True, apply_ct=True)
        c = bat.classify(b.h, E.EGRESS, E.EP, want_ct=True, apply_ct=True, seq=False)
        out.append((_differ(s, c), _differ(s, c, ct=True)))
    return out


_block_views = {}


def block_views(family, which):
    if (family, which) not in _block_views:
        blocks = E.pair_blocks(family) if which == "pairs" else E.triple_blocks(family)
        _block_views[family, which] = (blocks, _views(family, blocks))
    return _block_views[family, which]


# ordered pairs of the catalogue's kinds whose two views differ: in action,
# verdict or identity; with the CT byte counted too (measured)
DIFFERING_PAIRS = {4: (12, 75), 6: (6, 117)}


@pytest.mark.parametrize("family", FAMILIES)
def test_rule_sufficiency_over_pairs(family):
    """Every ordered pair of kinds from fresh CT state: a pair whose second
    header in packet order differs from the batch-start view — in action,
    verdict or identity, or in its CT byte — is cut by the rule.

    An earlier probe of 57 / 58 kinds to the endpoint's own address alone
    found 105 / 54 pairs differing in action, verdict or identity.  This
    catalogue (24 / 25 kinds, 576 / 625 pairs) has 12 / 6 such pairs: the
    endpoint's own ingress admits only TCP 80 and UDP 53 from itself, so a
    verdict turns on CT state only for the answers (SYN-ACK, RST, UDP back,
    echo reply, the answer to IPV4_LOOPBACK) of the few kinds that open a
    flow.  With the CT byte counted the views differ on 75 / 117 pairs whose
    second header is listed; the GPU tests compare that byte too.  Both counts are asserted as
    measured, the sets are named in the failure message."""
    blocks, diff = block_views(family, "pairs")
    t = E.env(family).t
    n_cut, differ, differ_ct, uncut = 0, [], [], []
    for b, (d, dc) in zip(blocks, diff):
        cuts = E.expected_cuts(t, b.h)
        assert cuts in ([], [1])
        n_cut += len(cuts)
        assert set(d) <= set(dc) <= {1}, (b.names, d, dc)
        if len(d):
            differ.append(b.names)
        # (a never-listed flow's second packet differs in its CT byte as well:
        # the ordering passes' business, ctorder.hip, not the cuts')
        if len(dc) and E.listed_rows(t, b.h.slice(1, 2))[0]:
            differ_ct.append(b.names)
            if not cuts:
                uncut.append(b.names)
    print(f"v{family}: {len(blocks)} pairs, {len(differ)} differ, {len(differ_ct)} with the "
          f"CT byte, {n_cut} cut")
    assert not uncut, uncut
    assert (len(differ), len(differ_ct)) == DIFFERING_PAIRS[family], (differ, len(differ_ct))


@pytest.mark.parametrize("family", FAMILIES)
def test_triples_hold_their_dependency(family):
    """In every triple the third header's packet-order result differs from
    the batch-start view (it depends on the first), in the CT byte at least;
    triples of both shapes exist: the middle header cut, and not listed"""
    blocks, diff = block_views(family, "triples")
    t = E.env(family).t
    dependent, mid_cut, mid_unlisted = 0, 0, 0
    for b, (d, dc) in zip(blocks, diff):
        cuts = E.expected_cuts(t, b.h)
        rows, _ = E.listed_rows(t, b.h)
        listed = {r[0] for r in rows}
        if 2 in dc:
            dependent += 1
            mid_cut += 1 in cuts
            if 1 not in listed:
                mid_unlisted += 1
                assert cuts == [2], (b.names, cuts)
        for j in dc:
            assert any(c <= j for c in cuts), (b.names, dc, cuts)
    print(f"v{family}: {len(blocks)} triples, {dependent} dependent, {mid_cut} behind a cut, "
          f"{mid_unlisted} across an unlisted header")
    assert dependent >= 24 and mid_cut >= 12 and mid_unlisted >= 6


def _seq(c, clock=E.BASE_CLOCK):
    o = O.Oracle(c.t)
    o.set_clock(clock)
    return o.classify(c.h, c.mode, c.ep, want_ct=True, apply_ct=True), o.ct_dump()


def _batch_start(c, clock=E.BASE_CLOCK):
    o = O.Oracle(c.t)
    o.set_clock(clock)
    return o.classify(c.h, c.mode, c.ep, nthreads=8, want_ct=True)


def _segments(c, cuts, clock=E.BASE_CLOCK):
    """each segment looked up at its start and folded before the next"""
    o = O.Oracle(c.t)
    o.set_clock(clock)
    parts = [o.classify(c.h.slice(a, b), c.mode, c.ep, want_ct=True, apply_ct=True, seq=False)
             for a, b in zip([0] + cuts, cuts + [len(c.h)])]
    return [np.concatenate([p[k] for p in parts]) for k in range(4)], o.ct_dump()


def _small_cases(family):
    c = dict(E.cut_cases(family))
    c.update(E.address_cases(family))
    c.update(E.no_cut_cases(family))
    return c


@pytest.mark.parametrize("family", FAMILIES)
def test_segment_counts_and_dependencies(family):
    """Every small stream of the GPU tests: cuts where the test claims them,
    none where it claims one launch; a cut stream differs somewhere from its
    batch-start view (the cuts matter), and its segments — each looked up at
    its start, folded before the next — give the packet-order result header
    by header on every listed header (the cuts suffice)."""
    for name, c in _small_cases(family).items():
        cuts = E.expected_cuts(c.t, c.h, c.mode, c.ep)
        assert (len(cuts) > 0) == c.cut, (name, cuts)
        seq, rows = _seq(c)
        if c.cut:
            assert len(_differ(seq, _batch_start(c), ct=True)), name
        seg, seg_rows = _segments(c, cuts)
        # (a plain flow's second packet inside a segment is the ordering
        # passes' business, ctorder.hip, not the cuts': listed headers only)
        d = _differ(seq, seg, ct=True)
        listed = {r[0] for r in E.listed_rows(c.t, c.h, c.ep)[0]}
        assert not listed & set(d), (name, sorted(listed & set(d))[:8])
        if not len(d):
            np.testing.assert_array_equal(rows, seg_rows)
    c = E.cut_cases(family)
    assert len(E.expected_cuts(c["one_flow"].t, c["one_flow"].h)) == len(c["one_flow"].h) - 1
    n = len(c["edge_cuts"].h)
    assert E.expected_cuts(c["edge_cuts"].t, c["edge_cuts"].h) == [1, n - 1]


@pytest.mark.parametrize("family", FAMILIES)
def test_address_set_cases(family):
    """what each address-set stream is about"""
    c = E.address_cases(family)
    for name in ("svc_2", "svc_l3") + (("loopback",) if family == 4 else ()):
        rows, n_own = E.listed_rows(c[name].t, c[name].h)
        assert [r[0] for r in rows] == [0, 1, 3] and rows[0][3] >= n_own > rows[1][3]
        # without the service's address in the set the cut at 1 is not made
        assert E.cut_rule(rows[1:], n_own, family == 6) == [3]
    t = c["svc_2"].t
    lb = t.lb4 if family == 4 else t.lb6
    own = E.address_set(t, E.EP, family)[0][0]
    tgt = [bytes(np.asarray(x, np.uint8)) if family == 6 else int(x).to_bytes(4, "little")
           for x in lb["target"]]
    mine = [(int(r["slave"]), int(r["dport"])) for r, x in zip(lb, tgt) if x == own and r["slave"]]
    assert any(s >= 2 and p for s, p in mine) and any(s >= 2 and not p for s, p in mine)
    rows, _ = E.listed_rows(c["no_services"].t, c["no_services"].h)
    assert len(rows) == 2 and E.address_set(c["no_services"].t, E.EP, family)[1] == []
    assert E.listed_rows(c["no_address"].t, c["no_address"].h) == ([], 0)
    assert c["second_endpoint"].ep != E.EP
    assert E.listed_rows(c["second_endpoint"].t, c["second_endpoint"].h,
                         c["second_endpoint"].ep)[0] == []
    # the same headers from the endpoint itself are cut before every one
    h = E.one_flow(family, 20)
    assert len(E.expected_cuts(E.env(family).t, h)) == 19


@pytest.mark.parametrize("family", FAMILIES)
def test_ingress_batches_need_no_cut(family):
    """ingress batches are never cut.  The self-addressed stream
    arriving at the endpoint (INGRESS) and in FULL mode: packet order and
    the batch-start view agree in action, verdict and identity on every
    header — while the same stream as the endpoint's egress batch does not."""
    c = E.no_cut_cases(family)
    for name in ("ingress", "full"):
        assert len(_differ(_seq(c[name])[0], _batch_start(c[name]))) == 0, name
    eg = E.Case(c["ingress"].t, c["ingress"].h)
    assert len(_differ(_seq(eg)[0], _batch_start(eg))) > 0


@pytest.mark.parametrize("family", FAMILIES)
def test_structural_stream(family):
    """n = 8192 * 256 + 257; listed headers at 0, 1, 63, 64, 255, 256,
    2 097 151, 2 097 152 and n-1 among others; on each side of every
    boundary a header whose packet-order result differs from its batch-start
    one (IPv4: in its verdict; IPv6, where the answer of a flow to itself is
    dropped in both views, in its CT byte); the 130-run holds none"""
    h, at = E.structural_stream(family)
    c = E.Case(E.env(family).t, h)
    n = len(h)
    assert n == 8192 * 256 + 257
    assert set([0, 1, 63, 64, 255, 256, E.GRID - 1, E.GRID, n - 1]) <= set(at)
    rows, _ = E.listed_rows(c.t, h)
    assert [r[0] for r in rows] == at
    cuts = E.expected_cuts(c.t, h)
    assert cuts == [1, 62, 64, 254, 256, E.GRID - 2, E.GRID, n - 1]
    seq, bat = _seq(c)[0], _batch_start(c)
    d = _differ(seq, bat, ct=True)
    dv = _differ(seq, bat)
    for b in E.BOUNDARIES:
        assert b in d and (b == 1 or b - 2 in d), (b, d[:20])
        if family == 4:
            assert b in dv and (b == 1 or b - 2 in dv), (b, dv[:20])
    assert n - 1 in d
    run = np.arange(E.RUN[0], E.RUN[0] + E.RUN[1])
    assert set(run) <= set(at) and not set(run) & set(d)
    assert E.RUN[0] % 64 and (E.RUN[0] + E.RUN[1]) % 64 and E.RUN[1] > 128


@pytest.mark.parametrize("family", FAMILIES)
def test_ragged_and_growth_streams(family):
    """the ragged schedule over a self stream: most scheduled batches are cut
    again inside; the growth stream's first cut comes after all its plain
    new flows"""
    import ct_edge_streams as CE
    from test_gpu_self import _self_stream
    c = E.ragged_self(family, _self_stream, sum(CE.SIZES))
    per = [len(E.expected_cuts(c.t, c.h.slice(a, b))) for a, b in CE.cuts(CE.SIZES)]
    assert sum(1 for x in per if x) >= 8 and per[-1] > 1000, per
    g = E.growth_case(family)
    cuts = E.expected_cuts(g.t, g.h)
    assert cuts[0] == 6001 and len(cuts) == 39
    o = O.Oracle(g.t)
    o.set_clock(E.BASE_CLOCK)
    before = len(o.ct_dump())
    o.classify(g.h.slice(0, cuts[0]), E.EGRESS, E.EP, apply_ct=True)
    assert len(o.ct_dump()) > 8 * before, (before, len(o.ct_dump()))
