#!/usr/bin/env python3
"""Times of the params-file path (halo2_vectordb_amd/srs.py): ParamsKZG.read(path, k) of a large file downsized to k, and
vdb_g1_lagrange_from_monomial_dev alone (at the file's own k no downsize runs, so a k = 22 user pays it only when cutting down).

    python tools/srs_downsize_bench.py --dir SCRATCH [--file-k 22] [--read-ks 16,18,20] [--dft-ks 16,18,20,22] [--reps 3] [--out x.json]

Writes the unsafe-setup file of --file-k into SCRATCH (2^(k+1) x 64 B: 512 MiB at k = 22) and removes it at the end.  Every size is
run once untimed first.  read_s: host clock around the whole read (file I/O, point checks, downsize, copies — it ends in a D2H copy,
so the device has finished); dft_call_ms: device events around the one call (its work-buffer allocation included); dft_kernel_ms:
the sum of its kernels' HIP-event times (vdb_profile_begin).  model_ms: the issue's model — 4.3 k field products per scalar
multiplication (254 doublings of ~10 products, ~127 additions of ~14) for the (n/2) k - (n - 1) non-trivial butterflies and the n
products by n^-1 — at the product rate vdb_bench_fr_mul measures in the same process."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from halo2_vectordb_amd import _lib, api  # noqa: E402
from halo2_vectordb_amd.srs import ParamsKZG  # noqa: E402

PRODUCTS_PER_SCALAR_MUL = 254 * 10 + 127 * 14


def scalar_muls(k):
    n = 1 << k
    return (n // 2) * k - (n - 1) + n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True)
    ap.add_argument("--file-k", type=int, default=22)
    ap.add_argument("--read-ks", default="16,18,20")
    ap.add_argument("--dft-ks", default="16,18,20,22")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    read_ks = [int(x) for x in a.read_ks.split(",") if x]
    dft_ks = [int(x) for x in a.dft_ks.split(",") if x]
    api.init(0)
    lib = _lib.init()
    rate = api.bench_fr_mul()
    res = dict(file_k=a.file_k, fr_mul_per_s=rate, products_per_scalar_mul=PRODUCTS_PER_SCALAR_MUL, read={}, dft={})
    path = os.path.join(a.dir, f"kzg_bn254_{a.file_k}.srs")
    t0 = time.perf_counter()
    params = ParamsKZG.setup_unsafe(a.file_k, None)
    params.write(path)
    res["write_file_s"] = time.perf_counter() - t0
    try:
        for k in read_ks:
            ParamsKZG.read(path, k)
            times = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                p = ParamsKZG.read(path, k)
                times.append(time.perf_counter() - t0)
            assert np.array_equal(p.g, params.g[: 1 << k])
            res["read"][k] = dict(read_s=min(times), read_s_all=times)
            print("read", k, res["read"][k], flush=True)
        for k in dft_ks:
            n = 1 << k
            d = api.DeviceBuffer(n * 64)
            o = api.DeviceBuffer(n * 64)
            try:
                d.upload(params.g[:n])
                _lib.check(lib.vdb_g1_lagrange_from_monomial_dev(k, d.ptr, o.ptr))
                calls = []
                for _ in range(a.reps):
                    api.timer_start()
                    _lib.check(lib.vdb_g1_lagrange_from_monomial_dev(k, d.ptr, o.ptr))
                    calls.append(api.timer_stop())
                api.profile_begin()
                _lib.check(lib.vdb_g1_lagrange_from_monomial_dev(k, d.ptr, o.ptr))
                prof = api.profile_end()
                kernels = [sum(v["ms"] for name, v in prof.items() if name.startswith("k_g1_dft"))]
                if k == a.file_k:
                    assert np.array_equal(o.download((n, 8)), params.g_lagrange)
                model_ms = scalar_muls(k) * PRODUCTS_PER_SCALAR_MUL / rate * 1e3
                res["dft"][k] = dict(dft_call_ms=min(calls), dft_kernel_ms=min(kernels), model_ms=model_ms,
                                     model_over_kernel=model_ms / min(kernels), per_kernel_ms={name: v["ms"] for name, v in prof.items()})
                print("dft", k, {key: v for key, v in res["dft"][k].items() if key != "per_kernel_ms"}, flush=True)
            finally:
                d.free()
                o.free()
    finally:
        os.remove(path)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
