"""What it costs to make a batch's proxy-map entries visible to the from-host
lookups (GPU box), on a cilium_proxy4 map of 100 k entries and a batch of 1 M
IPv4 headers of which 10 k are redirected, every one with a key the map does
not hold yet:

  commit   CFC_PROXY_APPLY_COMMIT (the default): cfc_proxy_apply_v4, then the
           cfc_commit that re-flattens the map and uploads the table
  device   CFC_PROXY_APPLY_DEVICE: cfc_proxy_apply_v4 alone, which folds its
           records into the live table on the device

Each case runs in a process of its own under a time limit: two warm-up
batches, then --reps timed ones (wall clock around the calls, which
synchronise the stream themselves; every batch brings new keys, so the map
grows by 10 k per batch in both cases).  After the last batch a from-host
batch over that batch's keys must hit every one of them.  Prints one JSON
line per case and writes them, with the medians, to --out/ab.json.

  python3 scripts/proxy_apply_ab.py [--out DIR] [--reps 5] [--timeout 300]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PROXY_PORT = 0x1127            # 10001, be16 raw


def case(a):
    import numpy as np
    import torch
    from cilium_amd import _lib as L
    from cilium_amd import synth as S
    from cilium_amd.datapath import Datapath, HeaderBatchV4, Verdicts
    from cilium_amd.loader import load_tables

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    rounds = a.warmup + a.reps
    total = a.entries + rounds * a.redirects
    # distinct keys {saddr, the proxy port, sport, TCP}: the map's, then each batch's
    sa = rng.permutation(np.unique(rng.integers(1 << 24, 1 << 32, size=2 * total,
                                                dtype=np.uint64).astype(np.uint32)))[:total]
    sp = rng.integers(1024, 65536, size=total).astype(np.uint32)
    assert len(sa) == total

    def keys_vals(lo, hi):
        m = hi - lo
        k = np.zeros((m, 10), np.uint8)
        k[:, 0:4] = sa[lo:hi].astype("<u4").view(np.uint8).reshape(m, 4)
        k[:, 4:8] = (np.uint32(PROXY_PORT) | sp[lo:hi] << np.uint32(16)).astype("<u4") \
            .view(np.uint8).reshape(m, 4)
        k[:, 8] = 6
        v = np.zeros((m, 16), np.uint8)
        v[:, 0:4] = rng.integers(1, 255, size=(m, 4))
        v[:, 4:6] = rng.integers(1, 255, size=(m, 2))
        return k, v

    dp = Datapath(0)
    load_tables(dp, S.config_c2(2, n_prefixes=4000, n_policy=1024, n_endpoints=2))
    dp.set_clock(1000)
    if a.case == "device":
        dp.set_option(L.OPT_PROXY_APPLY, L.PROXY_APPLY_DEVICE)
    dp.update_batch(dp.proxy.fd4, *keys_vals(0, a.entries))
    dp.commit()
    slots0 = dp.proxy_table_stats(False)["slots"]

    def t32(x):
        return torch.from_numpy(np.ascontiguousarray(x, np.uint32).view(np.int32)).to(dev)

    n = a.headers
    ms = []
    for r in range(rounds):
        lo = a.entries + r * a.redirects
        rows = np.sort(rng.choice(n, size=a.redirects, replace=False))
        s = rng.integers(1 << 24, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        p = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        s[rows] = sa[lo:lo + a.redirects]
        p[rows] = sp[lo:lo + a.redirects] | np.uint32(0x5000) << np.uint32(16)
        ver = np.zeros(n, np.int32)
        ver[rows] = PROXY_PORT
        b = HeaderBatchV4(t32(s), t32(np.full(n, 0x0100000A, np.uint32)), t32(p),
                          t32(np.full(n, 6 | 100 << 16, np.uint32)))
        out = Verdicts(torch.from_numpy(ver).to(dev),
                       torch.zeros(n, dtype=torch.int32, device=dev), None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = dp.proxy_apply(b, out, L.MODE_INGRESS, 0)
        if a.case == "commit":
            dp.commit()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        assert st["created"] == a.redirects and st["failed"] == 0, st
        if r >= a.warmup:
            ms.append((t1 - t0) * 1e3)
    # the last batch's keys, as the proxy's packets come back: every one hits
    m = a.redirects
    lo = a.entries + (rounds - 1) * m
    pb = HeaderBatchV4(t32(np.full(m, 0x0100000B, np.uint32)), t32(sa[lo:lo + m]),
                       t32(np.uint32(PROXY_PORT) | sp[lo:lo + m] << np.uint32(16)),
                       t32(np.full(m, 6 | 100 << 16, np.uint32)),
                       torch.zeros(m, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    _, tr = dp.classify_from_host(pb)
    torch.cuda.synchronize()
    hits = int(tr.hits.item())
    ts = dp.proxy_table_stats(False)
    dp.close()
    assert hits == m, (hits, m)
    print(json.dumps(dict(case=a.case, entries=a.entries, headers=n, redirects=m,
                          call_ms=[round(x, 3) for x in ms],
                          median_ms=round(statistics.median(ms), 3),
                          table_bytes_start=20 * slots0, table_bytes_end=20 * ts["slots"],
                          patched=ts["patched"], rebuilt=ts["rebuilt"], hits=hits)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["commit", "device"], default=None)
    ap.add_argument("--entries", type=int, default=100_000)
    ap.add_argument("--headers", type=int, default=1 << 20)
    ap.add_argument("--redirects", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "proxy_apply"))
    a = ap.parse_args()
    if a.case:
        return case(a)
    results = []
    for name in ("commit", "device"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name,
                            "--entries", str(a.entries), "--headers", str(a.headers),
                            "--redirects", str(a.redirects), "--reps", str(a.reps),
                            "--warmup", str(a.warmup)],
                           capture_output=True, text=True, timeout=a.timeout)
        if r.returncode:
            sys.stderr.write(r.stdout + r.stderr)
            return r.returncode
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ab.json"), "w") as f:
        json.dump(dict(results=results,
                       median_ms={r["case"]: r["median_ms"] for r in results}), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
