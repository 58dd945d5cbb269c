"""The arithmetic tests/hist_wide.py restates, against the sources, and the
properties its shapes are chosen for (tests/test_gpu_hist_wide.py runs them):
that the dense sizes end on every side of a lane's 16 bytes, of its step and
of a workgroup's step; that the compact-region batch has three slices and a
region cut by a slice edge with live words on both sides; that the escape
batch overflows both fields of a slot inside one slice.  k_hist's step is
the 16 bytes it was before these tests (W = 1: wider steps were measured
slower and are not in the library), so the sizes around 4 W repeat 3, 4, 5
and the dense and region cases lie close to those of
tests/test_gpu_key_compact.py; what is new here is the reduce's alignment
rule and its split of a group's rows over the waves.  No GPU."""
import re

import numpy as np

import hist_wide as H


def _squeezed(name):
    """the source without white space: an expression is found however it is laid out"""
    return re.sub(r"\s+", "", H._source(name))


def test_constants_match_the_sources():
    hip, hpp = _squeezed("classify.hip"), _squeezed("classify.hpp")
    assert H.constant("classify.hpp", "BLOCK") == H.BLOCK
    assert "KEY_WAVES=BLOCK/64;" in hpp
    # hist_slices, hist_per_block, hist_reduce_vec as restated in hist_wide.py
    assert "nb=std::min<uint64_t>(256,(n+4095)/4096);" in hip
    assert "return(pb+3)&~3ull;" in hip
    assert "return((poff|cnt)&3)==0;" in hip
    # a group of the reduce is whole unrolled passes of its waves
    assert H.reduce_rows() % (H.REDUCE_WAVES * H.REDUCE_UNROLL) == 0


def test_dense_sizes_cover_the_step_edges():
    sizes = H.dense_sizes()
    s = H.STEP
    assert {n % 4 for n in sizes} == {0, 1, 3}
    assert {s - 1, s, s + 1} <= set(sizes)
    # a workgroup's step is 1024 lanes wide: one word short of it, one past
    # it (a second slice), and two steps and a scalar tail
    assert 1024 * s - 1 in sizes and 1024 * s + 1 in sizes and 2 * 1024 * s + 3 in sizes
    # slices of the dense identity job at these sizes: one, and more than one
    # whose last is partial
    nb = {n: H.hist_slices(n, 1000) for n in sizes}
    assert nb[1] == 1 and nb[sizes[-1]] > 1
    n = sizes[-1]
    assert H.hist_per_block(n, nb[n]) * nb[n] > n


def test_region_batch_geometry():
    n = H.N_REGIONS
    assert H.key_per_block(n) == H.BLOCK and H.CAP == 64
    ext = H.key_extent(n)
    assert ext == 10 * H.BLOCK
    assert H.hist_slices(n, 1000) == 3
    per = H.hist_per_block(ext, 3)
    # the first slice edge cuts region STRADDLE with live words on both sides
    r, at = divmod(per, H.CAP)
    assert r == H.STRADDLE and 0 < at < H.STRADDLE_LIVE
    counts = H.region_counts()
    s = H.STEP
    assert {0, 1, s - 1, s, s + 1, H.CAP} <= set(counts.values())
    kinds = H.region_kinds()
    for r, live in counts.items():
        assert np.count_nonzero(kinds[H.CAP * r:H.CAP * (r + 1)] == H.BOTH) == live
    # the regions behind the named ones are a mix (ragged counts)
    rest = kinds[H.CAP * 7:H.CAP * H.STRADDLE].reshape(-1, H.CAP)
    assert len({int(np.count_nonzero(x == H.BOTH)) for x in rest}) > 5


def test_escape_batch_overflows_both_fields_in_one_slice():
    kinds = H.hot_interleaved()
    n, hot = len(kinds), int(np.count_nonzero(kinds == H.BOTH))
    assert H.hist_slices(n, 1000) == 1
    assert hot > 2047 and hot * 1500 >= 1 << 21
    # a lane's 16 bytes of the dense stream: the hot key three times
    assert all(np.count_nonzero(kinds[i:i + 4] == H.BOTH) == 3 for i in range(0, n, 4))


def test_reduce_rule_and_slices():
    assert H.reduce_vec(0, 512) and not H.reduce_vec(0, 510)
    assert not H.reduce_vec(3 * 510, 36864) and H.reduce_vec(4 * 510, 36864)
    assert H.hist_slices(4096, 1000) == 1 and H.hist_slices(10_000, 1000) == 3
    # rows a wave of the reduce takes (every REDUCE_WAVES-th of the group):
    # one slice leaves waves without a row, three slices too; 33 slices give
    # the first wave one row more than an unrolled pass
    rows = lambda nblk, wave: len(range(wave, min(nblk, H.reduce_rows()), H.REDUCE_WAVES))   # noqa: E731
    assert [rows(1, w) for w in range(H.REDUCE_WAVES)] == [1, 0, 0, 0]
    assert [rows(3, w) for w in range(H.REDUCE_WAVES)] == [1, 1, 1, 0]
    assert H.hist_slices(33 * 4096 - 5, 1000) == 33
    assert rows(33, 0) == H.REDUCE_UNROLL + 1 and rows(33, 1) == H.REDUCE_UNROLL
