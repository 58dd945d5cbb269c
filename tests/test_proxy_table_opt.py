"""CFC_OPT_PROXY_APPLY and cfc_proxy_table_stats without a GPU: the binding,
the error returns on a host-only context, the ABI version; the Python
restatement of the reverse-proxy tables' hashes (rp_table.py) against
layout.h; and what the key sets of test_gpu_proxy_table.py claim about
themselves — home slots, cluster positions, the wrap."""
import ctypes
import errno
import os
import shutil
import subprocess

import numpy as np
import pytest

import revproxy_streams as RS
import rp_table as T
from cilium_amd import _lib as L
from cilium_amd.datapath import host_only

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMS = pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])


# ------------------------------------------------------------------ the ABI
def test_option_and_symbol_bound():
    assert (L.OPT_PROXY_APPLY, L.PROXY_APPLY_COMMIT, L.PROXY_APPLY_DEVICE) == (7, 0, 1)
    assert "cfc_proxy_table_stats" in L.EXPORTS
    lib = L.lib()
    assert lib.cfc_proxy_table_stats.argtypes is not None
    assert ctypes.sizeof(L.ProxyTableStat) == 40
    assert [f for f, _ in L.ProxyTableStat._fields_] == \
        ["slots", "entries", "patched", "rebuilt", "inserted", "updated"]
    hdr = open(os.path.join(ROOT, "include", "cfc.h")).read()
    for word in ("#define CFC_OPT_PROXY_APPLY 7", "#define CFC_PROXY_APPLY_COMMIT 0",
                 "#define CFC_PROXY_APPLY_DEVICE 1", "cfc_proxy_table_stat;",
                 "int cfc_proxy_table_stats(cfc_ctx *ctx, int family, cfc_proxy_table_stat *st);"):
        assert word in hdr


def test_abi_version_stays_13():
    assert L.lib().cfc_abi_version() == 13
    assert ctypes.sizeof(L.ProxyStats) == 40


def test_option_values():
    dp = host_only()
    try:
        dp.set_option(L.OPT_PROXY_APPLY, L.PROXY_APPLY_DEVICE)
        dp.set_option(L.OPT_PROXY_APPLY, L.PROXY_APPLY_COMMIT)
        for bad in (2, -1, 1 << 32):
            with pytest.raises(OSError) as e:
                dp.set_option(L.OPT_PROXY_APPLY, bad)
            assert e.value.errno == errno.EINVAL
    finally:
        dp.close()


def test_table_stats_errors_on_a_host_only_context():
    dp = host_only()
    try:
        with pytest.raises(OSError) as e:
            dp.proxy_table_stats(False)
        assert e.value.errno == errno.ENODEV
        with pytest.raises(OSError) as e:
            dp.proxy_table_stats(True)
        assert e.value.errno == errno.ENODEV
        st = L.ProxyTableStat()
        for fam in (0, 5, 7, -4):
            assert dp.L.cfc_proxy_table_stats(dp.h, fam, ctypes.byref(st)) == -errno.EINVAL
        assert dp.L.cfc_proxy_table_stats(dp.h, 4, None) == -errno.EINVAL
        assert dp.L.cfc_proxy_table_stats(None, 4, ctypes.byref(st)) == -errno.EINVAL
    finally:
        dp.close()


# ------------------------------------------------------- the hash restatement
def test_hashes_against_layout_h(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert shutil.which(hipcc), "the HIP compiler the library is built with"
    exe = str(tmp_path / "rp_hash_host")
    subprocess.run([hipcc, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function",
                    "-I", os.path.join(ROOT, "cilium_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "c", "rp_hash_host.cpp")], check=True)
    rng = np.random.default_rng(11)
    edge = [0, 1, 0xFFFFFFFF, 0x80000000, 0x7ed55d16, 0x3c6ef372]
    v4 = [(a, b, c) for a in edge[:4] for b in edge[:3] for c in (0, 6, 17, 255)]
    v4 += [tuple(int(x) for x in rng.integers(0, 1 << 32, 2)) + (int(rng.integers(0, 256)),)
           for _ in range(40)]
    v6 = [(a, a, b, b, c, d) for a in edge[:4] for b in edge[:2] for c in edge[:3]
          for d in (0, 6, 255)]
    v6 += [tuple(int(x) for x in rng.integers(0, 1 << 32, 5)) + (int(rng.integers(0, 256)),)
           for _ in range(40)]
    text = "".join("4 " + " ".join(f"{x:x}" for x in v) + "\n" for v in v4) + \
        "".join("6 " + " ".join(f"{x:x}" for x in v) + "\n" for v in v6)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = [int(x, 16) for x in r.stdout.split()]
    want = [int(T.rp4_hash(*v)) for v in v4] + [int(T.rp6_hash(*v)) for v in v6]
    assert len(got) == len(v4) + len(v6) and got == want
    # ... and the vectorised form the key search uses
    a = np.array(v4, np.uint32)
    assert [int(x) for x in T.rp4_hash(a[:, 0], a[:, 1], a[:, 2])] == want[:len(v4)]
    b = np.array(v6, np.uint32)
    assert [int(x) for x in T.rp6_hash(*(b[:, i] for i in range(6)))] == want[len(v4):]


def test_key_words_and_sizing():
    k4 = T.key(False, bytes([1, 2, 3, 4]), 0x1234, 17)
    assert len(k4) == 10 and T.key_words(k4) == ((0x04030201,), T.PROXY_PORT | 0x1234 << 16, 17)
    k6 = T.key(True, bytes(range(16)), 0xBEEF)
    assert len(k6) == 22 and T.key_words(k6) == \
        ((0x03020100, 0x07060504, 0x0B0A0908, 0x0F0E0D0C), T.PROXY_PORT | 0xBEEF << 16, 6)
    assert [T.slots_for(n, False) for n in (0, 1, 33, 64, 65)] == [0, 2, 128, 128, 256]
    assert [T.slots_for(n, True) for n in (0, 1, 33, 64, 65)] == [0, 4, 256, 256, 512]


# ------------------------------------------------- the structural key sets
@FAMS
def test_edge_keys_meet_their_claims(v6):
    x = T.edges(v6)
    s = x.shape
    assert len(x.base) == 33 and T.slots_for(33, False) == T.SLOTS == 128
    at = T.place(x.base)
    used = set(at.values())
    assert len(used) == 33
    home = T.home
    # the wrapping cluster: 126, 127, 0 taken, 125 and 1 free
    assert sorted(at[k] for k in s["wrap"]) == [0, 126, 127] and not {125, 1, 2} & used
    assert home(s["new_wrap"]) == 127          # walks 127, 0, lands behind the wrap
    # a cluster of three with the new key's home at its head
    assert [at[k] for k in s["cluster"]] == [8, 9, 10] and not {7, 11, 12} & used
    assert home(s["new_head"]) == 8
    # three existing keys of one home: one sits two slots from it
    assert [home(k) for k in s["trio"]] == [16] * 3 and not {15, 19} & used
    assert sorted(at[k] for k in s["trio"]) == [16, 17, 18]
    assert at[s["displaced"]] - home(s["displaced"]) == 2
    # three new keys of one free home slot
    assert [home(k) for k in s["new24"]] == [24] * 3 and not set(range(23, 28)) & used
    # the identical re-write
    rows = T.records_of(v6, x.recs)
    assert rows[s["same"]] == x.base[s["same"]] and rows[s["displaced"]] != x.base[s["displaced"]]
    # the address / port pairs
    al = 16 if v6 else 4
    p0, p1, o = s["pair"][0], s["pair"][1], s["other"]
    assert p0[al:] == p1[al:] and p0[:al] != p1[:al]
    assert o[:al] == p0[:al] and o[al:al + 4] != p0[al:al + 4] and o[al + 4:] == p0[al + 4:]
    hs = sorted(home(k) for k in (p0, p1, o))
    assert all(96 <= h <= 120 for h in hs) and hs[1] - hs[0] >= 2 and hs[2] - hs[1] >= 2
    assert not set(range(95, 122)) & used
    # the batch: 257 headers, records at the wave and batch edges, new and
    # existing keys told apart, distinct keys
    keys = [k for k, _ in x.recs]
    assert len(set(keys)) == len(keys) == 10 and {0, 63, 64, 256} <= set(x.at)
    assert set(x.new) == set(keys) - set(x.base) and len(x.new) == 8
    assert set(x.old) == set(keys) & set(x.base) and len(x.old) == 2
    h, ver, ide = T.redirect_headers(v6, x.recs, 257, x.at)
    assert len(h) == 257 and (np.flatnonzero(ver > 0) == np.array(sorted(x.at))).all()
    # the table stays within half load, so the batch is patched in place
    assert 33 + len(keys) <= 64
    # after the batch every slot of the zones is as claimed, whatever order
    # the new keys of one home arrive in (the occupied set of linear probing
    # does not depend on it)
    after = set(T.place(list(x.base) + x.new).values())
    assert {11, 1, 24, 25, 26} <= after and len(after) == 41


@FAMS
def test_probe_batch_hits_exactly_its_keys(v6):
    import revproxy_ref as R
    x = T.edges(v6)
    now = dict(x.base)
    now.update(T.records_of(v6, x.recs))
    keys = sorted(now)
    h, hit, miss = T.probes(v6, keys)
    tr = R.translate(h, now, np.zeros(len(h), np.uint32))
    assert tr.hit[hit].all() and not tr.hit[miss].any()
    assert len(hit) == 41 and len(miss) == 4 * 41 + 9
    # every key hits with its own value
    al = 16 if v6 else 4
    for i, k in enumerate(keys):
        assert bytes(np.ascontiguousarray(tr.saddr[i]).view(np.uint8)) == now[k][:al]
        assert int(tr.l4word[i]) & 0xFFFF == int.from_bytes(now[k][al:al + 2], "little")
    # the near misses differ from their key in exactly one field
    word = h.sport.astype(np.uint32) | h.dport.astype(np.uint32) << 16
    for j, k in enumerate(keys):
        base = (bytes(np.ascontiguousarray(h.daddr[j]).view(np.uint8)), int(h.sport[j]),
                int(h.dport[j]), int(h.proto[j]))
        for f in range(4):
            i = len(keys) + 4 * j + f
            row = (bytes(np.ascontiguousarray(h.daddr[i]).view(np.uint8)), int(h.sport[i]),
                   int(h.dport[i]), int(h.proto[i]))
            assert [a != b for a, b in zip(row, base)] == [g == f for g in range(4)]
    assert len(word) == len(h)
    # against the map before the batch, only the base keys hit
    tr0 = R.translate(h, x.base, np.zeros(len(h), np.uint32))
    assert tr0.hit.sum() == 33


def test_expect_runs_on_the_probe_batch():
    """the composition the GPU tests compare against takes the batch (the
    translated sources lie outside every ipcache prefix)"""
    x = T.edges(False)
    h, hit, miss = T.probes(False, sorted(x.base))
    e = RS.expect(RS.small(False), x.base, h)
    assert e.extra["unlabelled"] and e.tr.hit[hit].all() and not e.tr.hit[miss].any()
    assert len(set(e.ver.tolist())) > 1        # forwarded and dropped rows both
