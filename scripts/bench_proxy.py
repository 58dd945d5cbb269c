"""Cost of cfc_proxy_entries_v4 (GPU box), beside cfc_monitor_events_v4 on the
same batch — the existing ordered compaction of similar shape:
  (a) c2   the C2 bench batch (the bench's own tables, whose gen_policy has
           proxy_frac 0.05), classified in FULL mode
  (b) hot  every header redirected, flows Zipf(1.1) over 100 k keys (an L7
           policy's steady state: hand-made outputs, the calls read them as
           they stand)
each with the LDS pre-dedup and with it bypassed (CFC_PROXY_NO_PREDUP), in
alternated pairs.  The calls run on preallocated buffers; a timing covers the
whole call — its kernels, memsets and the one host wait that sizes the table —
between two device events.  Prints one JSON line per measurement and writes
them to --out.

  python3 scripts/bench_proxy.py [--headers N] [--steps K] [--out FILE]
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
    ap.add_argument("--keys", type=int, default=100_000)
    ap.add_argument("--cap", type=int, default=1 << 22)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from cilium_amd import _lib as L
    from cilium_amd import synth as S
    from cilium_amd.datapath import (Datapath, HeaderBatchV4, Verdicts, _ptr, hdr_struct,
                                     out_struct)
    from cilium_amd.loader import load_tables

    dev = torch.device("cuda", 0)
    n, cap = a.headers, a.cap
    t = S.config_c2_bench(2)
    dp = Datapath(0)
    load_tables(dp, t)
    rec = torch.zeros((cap, 8), dtype=torch.int32, device=dev)
    idx = torch.zeros(cap, dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(fn, b, out, mode):
        L.check(fn(dp.h, ctypes.byref(hdr_struct(b)), ctypes.byref(out_struct(out)), mode, 0,
                   _ptr(rec), _ptr(idx), cap, _ptr(cnt), stream), "call")

    def timed(fn, b, out, mode):
        call(fn, b, out, mode)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            call(fn, b, out, mode)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps, int(cnt.item())

    results = []

    def emit(**kw):
        results.append(kw)
        print(json.dumps(kw), flush=True)

    def proxy_bytes(redirects, entries):
        # count: the verdicts; mark: the verdicts again and, per redirected
        # header, ct + meta + ports + saddr + daddr; the table (own u64 +
        # last u32 per slot) zeroed, then last read once; the bitmap zeroed,
        # read twice; per record 32 B + the 8 B index + the header words again
        slots = 1024
        while slots < 2 * redirects:
            slots <<= 1
        return dict(count=4 * n, mark=4 * n + 17 * redirects, table=16 * slots,
                    bitmap=3 * (n // 8), records=(32 + 8 + 21) * entries, slots=slots)

    def pair(label, b, out, mode, k):
        row = {}
        for predup in ((True, False) if k % 2 == 0 else (False, True)):   # alternated
            if predup:
                os.environ.pop("CFC_PROXY_NO_PREDUP", None)
            else:
                os.environ["CFC_PROXY_NO_PREDUP"] = "1"
            ms, total = timed(dp.L.cfc_proxy_entries_v4, b, out, mode)
            row["predup_ms" if predup else "bypass_ms"] = round(ms, 4)
            row["entries"] = total
        os.environ.pop("CFC_PROXY_NO_PREDUP", None)
        emit(stream=label, pair=k, headers=n, **row)
        return row

    # (a) the C2 bench batch
    s, d, p, m = S.gen_batch_v4_torch(t, n, 2000, dev)
    b = HeaderBatchV4(s, d, p, m, None)
    out = Verdicts(torch.empty(n, dtype=torch.int32, device=dev),
                   torch.empty(n, dtype=torch.int32, device=dev), None,
                   torch.empty(n, dtype=torch.uint8, device=dev),
                   torch.empty(n, dtype=torch.int32, device=dev))
    dp.classify_v4(b, 3, 0, out=out)
    torch.cuda.synchronize()
    redirects = int((out.verdict > 0).sum().item())
    ms_mon, events = timed(dp.L.cfc_monitor_events_v4, b, out, 3)
    row = pair("c2", b, out, 3, 0)
    emit(stream="c2", headers=n, redirects=redirects, monitor_events_ms=round(ms_mon, 4),
         monitor_events=events, monitor_bytes=8 * n + min(events, cap) * (6 * 4 + 32 + 8),
         proxy_bytes=proxy_bytes(redirects, row["entries"]))
    del s, d, p, m, b, out

    # (b) the hot stream: Zipf(1.1) over a.keys flows, every header redirected
    g = torch.Generator(device=dev)
    g.manual_seed(9)
    w = 1.0 / torch.arange(1, a.keys + 1, device=dev, dtype=torch.float64) ** 1.1
    cdf = torch.cumsum(w, 0) / w.sum()
    flow = torch.searchsorted(cdf, torch.rand(n, device=dev, dtype=torch.float64, generator=g))
    flow = flow.clamp_(max=a.keys - 1).to(torch.int32)
    saddr = (flow >> 4) + 0x0A000000              # (the address's byte order does not matter here)
    ports = (1024 + (flow & 15)) | (80 << 16)
    daddr = torch.randint(1, 1 << 20, (n,), device=dev, dtype=torch.int32, generator=g)
    meta = torch.full((n,), 6 | (100 << 16), dtype=torch.int32, device=dev)
    b = HeaderBatchV4(saddr.contiguous(), daddr, ports.contiguous(), meta, None)
    out = Verdicts(torch.full((n,), int(S.htons(10001)), dtype=torch.int32, device=dev),
                   torch.full((n,), 300, dtype=torch.int32, device=dev), None,
                   torch.full((n,), 5, dtype=torch.uint8, device=dev),
                   # one trace word per header (TRACE_TO_PROXY, length class 1):
                   # the yardstick writes a record for every header it has room for
                   torch.full((n,), (4 + 1) << 16 | 1 << 22, dtype=torch.int32, device=dev))
    ms_mon, events = timed(dp.L.cfc_monitor_events_v4, b, out, 0)
    rows = [pair("hot", b, out, 0, k) for k in range(3)]
    emit(stream="hot", headers=n, redirects=n, keys=a.keys, monitor_events_ms=round(ms_mon, 4),
         monitor_events=events, monitor_bytes=8 * n + min(events, cap) * (6 * 4 + 32 + 8),
         proxy_bytes=proxy_bytes(n, rows[0]["entries"]),
         predup_faster_in_all_pairs=all(r["predup_ms"] < r["bypass_ms"] for r in rows))
    dp.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
