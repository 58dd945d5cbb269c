"""Cost of cfc_classify_from_host_v4 (GPU box) beside cfc_classify_v4 INGRESS
on the same batch: 64 Mi IPv4 headers on the C2 bench tables, a zero mark
column (so every case runs the same kernel flavour as far as it can), 1 % of
the headers rewritten into the proxy's packets towards the local endpoint.

  (a) cfc_classify_v4 INGRESS
  (b) cfc_classify_from_host_v4, empty proxy map (no lookup kernel)
  (c) 100 k proxy entries, no header hitting, aliased columns
  (d) 100 k entries, the 1 % hitting, aliased columns
  (e) as (d) with separate output columns

Each case has a context of its own (the proxy table is per commit), all on
the same tables and batch.  A run is --steps calls, each between two device
events of its own (an aliased call rewrites the batch in place: the batch is
restored before every call, outside the events); three runs of each case,
alternated.  With CFC_OPT_TIMING the classify and counter kernels' share of a
call is known, so what is left of a call is the lookup pass (and its memset).
The pass must stream daddr, ports and meta, 12 B per header, when the columns
alias; separate columns add a read and a write of saddr, a write of ports and
a read and a write of mark: 32 B (28 B for a batch without a mark column; the
batch here has one).  Prints one JSON line per measurement and writes them to --out.

  python3 scripts/bench_revproxy.py [--headers N] [--steps K] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--headers", type=int, default=64 << 20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--entries", type=int, default=100_000)
    ap.add_argument("--hit", type=float, default=0.01)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from cilium_amd import _lib as L
    from cilium_amd import synth as S
    from cilium_amd.datapath import (Datapath, HeaderBatchV4, Translated, Verdicts, _ptr,
                                     hdr_struct, out_struct)
    from cilium_amd.loader import load_tables

    dev = torch.device("cuda", 0)
    n = a.headers
    t = S.config_c2_bench(2)
    ep = int(S.local_v4_addrs(t)[0])
    rng = np.random.default_rng(7)

    # the proxy's connections: {client = the endpoint, client port, proxy port}
    words = np.unique(rng.integers(0, 1 << 32, size=2 * a.entries, dtype=np.uint64)
                      .astype(np.uint32))
    words = rng.permutation(words)[:a.entries].copy()

    def entries(saddr):
        k = np.zeros((a.entries, 10), np.uint8)
        k[:, 0:4] = np.asarray(saddr, "<u4").reshape(-1, 1).view(np.uint8).reshape(-1, 4)
        k[:, 4:8] = words.view(np.uint8).reshape(-1, 4)
        k[:, 8] = 6
        v = np.zeros((a.entries, 16), np.uint8)
        v[:, 0:4] = rng.integers(0, 256, size=(a.entries, 4))
        v[:, 0] = 203                                   # (outside the C2 prefixes or not:
        v[:, 4:6] = rng.integers(1, 256, size=(a.entries, 2))   # the pass does not care)
        return k, v

    def context(keys_vals):
        dp = Datapath(0)
        dp.set_option(L.OPT_TIMING, 1)
        load_tables(dp, t)
        if keys_vals is not None:
            dp.update_batch(dp.proxy.fd4, *keys_vals)
        dp.commit()
        return dp

    ctx = dict(empty=context(None),
               miss=context(entries(np.full(a.entries, 0xFEFEFEFA, np.uint32))),   # 250.254.254.254
               hit=context(entries(np.full(a.entries, ep, np.uint32))))

    s, d, p, m = S.gen_batch_v4_torch(t, n, 2000, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    sel = torch.rand(n, device=dev, generator=g) < a.hit
    pick = torch.randint(0, a.entries, (n,), device=dev, generator=g)
    w = torch.from_numpy(words.view(np.int32)).to(dev)
    ep_i32 = int(np.array([ep], np.uint32).view(np.int32)[0])
    d = torch.where(sel, torch.full_like(d, ep_i32), d)
    p = torch.where(sel, w[pick], p)
    m = torch.where(sel, (m & ~0xFFFF) | 6, m)          # TCP, no flags
    mark = torch.zeros(n, dtype=torch.int32, device=dev)
    pristine = (s.clone(), p.clone(), mark.clone())
    b = HeaderBatchV4(s, d.contiguous(), p.contiguous(), m.contiguous(), mark)
    new = lambda dt=torch.int32: torch.empty(n, dtype=dt, device=dev)   # noqa: E731
    out = Verdicts(new(), new(), None)
    ident, hits = new(), torch.zeros(1, dtype=torch.int64, device=dev)
    alias = Translated(b, ident, hits)
    sep = Translated(HeaderBatchV4(new(), b.daddr, new(), b.meta, new()), ident, hits)

    def restore():
        b.saddr.copy_(pristine[0])
        b.ports.copy_(pristine[1])
        b.mark.copy_(pristine[2])

    cases = [("a", "empty", None), ("b", "empty", alias), ("c", "miss", alias),
             ("d", "hit", alias), ("e", "hit", sep)]

    # the C calls on prebuilt structs: no Python between the events but the call
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    hdr, o = hdr_struct(b), out_struct(out)

    def cols_of(tr):
        tb = tr.batch
        return L.RevproxyCols(_ptr(tb.saddr), _ptr(tb.ports), _ptr(tb.mark), _ptr(tr.identity),
                              _ptr(tr.hits))
    cols = {id(alias): cols_of(alias), id(sep): cols_of(sep)}

    def call(dp, tr):
        if tr is None:
            rc = dp.L.cfc_classify_v4(dp.h, ctypes.byref(hdr), ctypes.byref(o), L.MODE_INGRESS, 0,
                                      stream)
        else:
            rc = dp.L.cfc_classify_from_host_v4(dp.h, ctypes.byref(hdr),
                                                ctypes.byref(cols[id(tr)]), ctypes.byref(o),
                                                stream)
        L.check(rc, "call")

    results = []

    def emit(**kw):
        results.append(kw)
        print(json.dumps(kw), flush=True)

    def run(name, which, tr, k):
        dp = ctx[which]
        restore()
        call(dp, tr)                                   # warm-up (workspace, first launch)
        torch.cuda.synchronize()
        dp.timing_collect()
        ms = []
        for _ in range(a.steps):
            restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(dp, tr)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        tm = dp.timing_collect()
        tot = sum(ms) / len(ms)
        cls, cnt = tm["classify_ms"] / a.steps, tm["count_ms"] / a.steps
        nh = int(hits.item()) if tr is not None else 0
        byt = 0 if which == "empty" or tr is None else (12 if tr is alias else 32) * n
        rest = tot - cls - cnt
        emit(case=name, run=k, headers=n, hits=nh, call_ms=round(tot, 4),
             call_ms_min=round(min(ms), 4), call_ms_max=round(max(ms), 4),
             classify_ms=round(cls, 4), count_ms=round(cnt, 4), rest_ms=round(rest, 4),
             lookup_bytes=byt,
             lookup_gb_s=round(byt / rest / 1e6, 1) if byt and rest > 0 else None)

    for k in range(a.runs):
        order = cases if k % 2 == 0 else cases[::-1]    # alternated
        for name, which, tr in order:
            run(name, which, tr, k)
    by = {c[0]: [r["call_ms"] for r in results if r["case"] == c[0]] for c in cases}
    emit(summary={c: dict(min=min(v), max=max(v)) for c, v in by.items()},
         b_inside_spread_of_a=min(by["a"]) <= max(by["b"]) and min(by["b"]) <= max(by["a"]))
    for dp in ctx.values():
        dp.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
