"""Shapes for the counter kernels' wide step and streaming reduce
(cilium_amd/csrc/classify.hip k_hist / hist_compact / k_hist_reduce), shared
by tests/test_hist_wide.py (no GPU: the arithmetic restated here against the
sources and the properties the shapes are chosen for) and
tests/test_gpu_hist_wide.py (the counters against the oracle).

The geometry below is the library's on an MI355X (256 CUs, two classify
workgroups per CU) for batches of at most 512 Ki headers: a classify
workgroup takes 1024 consecutive headers and its wave w the 64 headers behind
64 * w, so region r of a compact key stream holds the live words of headers
[64 r, 64 r + 64) and has 64 words (classify.hpp key_regions)."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cilium_amd", "csrc")

BLOCK = 1024
KEY_WAVES = BLOCK // 64
NWG = 256 * 2            # classify workgroups that fill an MI355X
CAP = BLOCK // KEY_WAVES   # words of a region while a workgroup takes BLOCK headers
BOTH, DROP, DEAD = 0, 1, 2   # what a header bumps: policy entry + identity, identity, nothing
LENGTHS = np.array([0, 1, 59, 1500, 65534, 65535], np.uint16)


def _source(name):
    return open(os.path.join(CSRC, name)).read()


def constant(name, what):
    """the value of `constexpr ... what = <number>;` in a source file"""
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % what, _source(name))
    assert m, (name, what)
    return int(m.group(1))


REDUCE_WAVES = constant("classify.hip", "REDUCE_WAVES")     # waves of a k_hist_reduce workgroup
REDUCE_UNROLL = constant("classify.hip", "REDUCE_UNROLL")   # rows a lane loads before it adds


def reduce_rows():
    m = re.search(r"#ifndef CFC_REDUCE_ROWS\n#define CFC_REDUCE_ROWS (\d+) ", _source("classify.hip"))
    assert m, "classify.hip: the default of CFC_REDUCE_ROWS"
    return int(m.group(1))


# 16-byte rows of a lane's step in k_hist's inner loops: one, four returning
# LDS atomics and one look at their returns (steps of two and four rows were
# measured slower and are not in the library, DESIGN.md §4 "The counter reduce")
W = 1
STEP = 4 * W             # key words of a lane's step


# ---- classify.hip hist_slices / hist_per_block, classify.hpp key_per_block / key_regions
def hist_slices(n, slots):
    if not n or not slots:
        return 0
    nb = min(256, (n + 4095) // 4096)
    nb = min(nb, max(1, (256 << 20) // (4 * slots)))
    nb = max(nb, (n + (1 << 31) - 1) >> 31)
    return max(nb, 1)


def hist_per_block(n, nblk):
    return ((n + nblk - 1) // nblk + 3) & ~3


def key_per_block(n, nwg=NWG, step=BLOCK):
    pb = (n + nwg - 1) // nwg
    pb = (pb + step - 1) // step * step
    return min(pb, (1 << 30) // step * step)


def key_extent(n):
    pb = key_per_block(n)
    return (n + pb - 1) // pb * pb


def reduce_vec(poff, cnt):
    """k_hist_reduce takes a job four keys per thread (16-byte loads)."""
    return (poff | cnt) % 4 == 0


# ---- the shapes
def dense_sizes(w=W):
    """Batch sizes around a lane's 16 bytes, its step and a workgroup's step
    of a dense job."""
    s = 4 * w
    return [1, 3, 4, 5, s - 1, s, s + 1, 1024 * s - 1, 1024 * s + 1, 2 * 1024 * s + 3]


N_REGIONS = 10_000       # three histogram slices; region 53 straddles the first slice edge
STRADDLE = 53
STRADDLE_LIVE = 40


def region_counts(w=W):
    """{region: live headers} of the compact-region batch: the counts around
    a lane's step, an empty and a full region, and the straddling one."""
    s = 4 * w
    return {0: 0, 1: 1, 2: s - 1, 3: s, 4: s + 1, 5: CAP, 6: 0, STRADDLE: STRADDLE_LIVE}


def region_kinds(n=N_REGIONS, seed=21, w=W):
    """Header kinds of the compact-region batch: the regions region_counts
    names hold exactly that many BOTH headers (in random lanes, DEAD
    elsewhere), every other region a random mix."""
    rng = np.random.default_rng(seed)
    kinds = rng.integers(0, 3, size=n)
    for r, live in region_counts(w).items():
        k = np.full(CAP, DEAD)
        k[rng.permutation(CAP)[:live]] = BOTH
        kinds[CAP * r:CAP * (r + 1)] = k
    return kinds


def hot_interleaved(n=4000, hot=3000):
    """Kinds of the escape batch: `hot` BOTH headers among n, three of every
    four consecutive positions, so that a lane's 16 bytes of the dense
    identity stream carry the same key three times."""
    kinds = np.where(np.arange(n) % 4 != 3, BOTH, DEAD)
    assert np.count_nonzero(kinds == BOTH) == hot
    return kinds
