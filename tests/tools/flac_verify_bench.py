#!/usr/bin/env python3
"""What the FLAC checks cost: python tests/tools/flac_verify_bench.py [--songs 4096] [--json out.json]

The corpus of flac_bench.py: N "songs" from the bytes of tests/golden/s32_stereo_44_1_kHz.flac and testcue.flac, alternating.
Each figure is the median of 3 runs after a warm-up:
  (a) blissgpu_analyze_batch_flac -- the unverified call -- and the SHA-256 of its rows
  (b) blissgpu_analyze_batch_flac_verified with the CRC-16, and with the CRC-16 and the MD5; blissgpu_flac_verify_batch alike
  (c) flac_crc_kernel alone against flac_decode_kernel alone on the same frame table (HIP events around the device-to-device
      calls): both read every compressed byte once
  (d) flac_md5_kernel alone, one song = one lane: MB/s of the FLAC message per lane, and the extrapolation to a three-minute
      44.1 kHz 16-bit stereo song
--unverified-only [--lib PATH]: (a) alone, through PATH when given -- a build without the new entry points, such as the parent
commit's, for an A/B of the untouched path (run the two builds alternately, a process each).
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def median3(fn):
    fn()
    runs = [fn() for _ in range(3)]
    return statistics.median(runs), min(runs), max(runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=4096)
    ap.add_argument("--json", default="")
    ap.add_argument("--unverified-only", action="store_true")
    ap.add_argument("--lib", default="")
    args = ap.parse_args()
    import torch

    u64p, u32p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    names = ["s32_stereo_44_1_kHz.flac", "testcue.flac"]
    blobs = [np.fromfile(os.path.join(ROOT, "tests", "golden", n), np.uint8) for n in names]
    n, d = args.songs, 23
    out = np.empty((n, d), np.float32)
    status = np.zeros(n, np.int32)
    ptrs = (C.c_void_p * n)(*[blobs[i % 2].ctypes.data for i in range(n)])
    sizes = np.array([blobs[i % 2].size for i in range(n)], np.uint64)
    res = {"songs": n, "flac_GB": int(sizes.sum()) / 1e9}

    if args.unverified_only and args.lib:
        L = C.CDLL(args.lib, mode=C.RTLD_GLOBAL)
        L.blissgpu_analyze_batch_flac.restype = C.c_int
        L.blissgpu_analyze_batch_flac.argtypes = [C.POINTER(C.c_void_p), u64p, C.c_uint32, C.c_uint32, C.c_void_p, i32p]
    else:
        from bliss_rs_amd import _ffi

        L = _ffi.lib()

    def unverified():
        t0 = time.perf_counter()
        rc = L.blissgpu_analyze_batch_flac(ptrs, sizes.ctypes.data_as(u64p), n, 2, out.ctypes.data, status.ctypes.data_as(i32p))
        assert rc == 0
        return time.perf_counter() - t0

    res["a_unverified_seconds"], res["a_min"], res["a_max"] = median3(unverified)
    res["a_rows_sha256"] = hashlib.sha256(out.tobytes()).hexdigest()
    rows = out.copy()
    if args.unverified_only:
        return finish(res, args)

    import bliss_rs_amd as bliss

    flags = np.zeros(n, np.uint32)
    first_bad = np.zeros(n, np.uint32)
    digests = np.zeros((n, 16), np.uint8)

    def verified(checks):
        def run():
            t0 = time.perf_counter()
            _ffi.check(L.blissgpu_analyze_batch_flac_verified(ptrs, sizes.ctypes.data_as(u64p), n, 2, checks, out.ctypes.data,
                                                              status.ctypes.data_as(i32p), flags.ctypes.data_as(u32p), first_bad.ctypes.data_as(u32p)))
            return time.perf_counter() - t0
        return run

    def verify_only(checks):
        def run():
            t0 = time.perf_counter()
            _ffi.check(L.blissgpu_flac_verify_batch(ptrs, sizes.ctypes.data_as(u64p), n, checks, flags.ctypes.data_as(u32p),
                                                    first_bad.ctypes.data_as(u32p), C.c_void_p(digests.ctypes.data)))
            return time.perf_counter() - t0
        return run

    for key, checks in (("crc", 1), ("crc_md5", 3)):
        res[f"b_analyze_verified_{key}_seconds"] = median3(verified(checks))[0]
        res[f"b_rows_equal_a_{key}"] = bool(np.array_equal(rows.view(np.uint32), out.view(np.uint32)))
        res[f"b_flags_{key}"] = sorted(set(int(f) for f in flags))
        res[f"b_verify_batch_{key}_seconds"] = median3(verify_only(checks))[0]
    res["d_md5_stage_corpus_seconds"] = res["b_verify_batch_crc_md5_seconds"] - res["b_verify_batch_crc_seconds"]

    # (c) / (d): a file repeated inside ONE table, as flac_bench.py does
    ctx = bliss.Context(0)
    res["c_kernels"], res["d_md5_lane"] = {}, {}
    for name, b in zip(names, blobs):
        info = np.zeros(_ffi.FLAC_INFO_WORDS, np.uint64)
        nf = C.c_uint64(0)
        L.blissgpu_flac_index(C.c_void_p(b.ctypes.data), b.size, 0, info.ctypes.data_as(u64p), None, 0, C.byref(nf))
        tab = np.zeros((nf.value, 4), np.uint64)
        L.blissgpu_flac_index(C.c_void_p(b.ctypes.data), b.size, 0, info.ctypes.data_as(u64p), tab.ctypes.data_as(u64p), nf.value, C.byref(nf))
        reps = max(1, min(n // 2, 512))
        stride = (b.size + 16 + 15) // 16 * 16
        host = np.zeros(reps * stride + 16, np.uint8)
        big = np.zeros((reps * len(tab), 4), np.uint64)
        total, ch, bps = int(info[3]), int(info[1]), int(info[2])
        for r in range(reps):
            host[r * stride:r * stride + b.size] = b
            big[r * len(tab):(r + 1) * len(tab)] = tab
            big[r * len(tab):(r + 1) * len(tab), 0] += np.uint64(r * stride)
            big[r * len(tab):(r + 1) * len(tab), 2] += np.uint64(r * total)
        info2 = info.copy()
        info2[3] = reps * total
        d_bytes = torch.from_numpy(host).cuda()
        d_pcm = torch.zeros((reps * total, ch), dtype=torch.int32 if bps > 16 else torch.int16, device="cuda")
        d_st = torch.zeros(len(big), dtype=torch.int32, device="cuda")
        d_end = torch.zeros(len(big), dtype=torch.int64, device="cuda")
        d_ok = torch.zeros(len(big), dtype=torch.int32, device="cuda")
        d_md5 = torch.zeros(16, dtype=torch.uint8, device="cuda")

        def timed(call):
            def run():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ctx._pre()   # (the context's stream waits for e0's stream and hands back to it: the events bracket the launch)
                _ffi.check(call())
                ctx._post()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) * 1e-3
            return run

        t_dec = median3(timed(lambda: L.blissgpu_flac_decode_device(
            ctx._h, C.c_void_p(d_bytes.data_ptr()), host.size - 16, big.ctypes.data_as(u64p), len(big), info2.ctypes.data_as(u64p),
            C.c_void_p(d_pcm.data_ptr()), C.c_void_p(d_st.data_ptr()), C.c_void_p(d_end.data_ptr()))))[0]
        assert int(d_st.abs().sum()) == 0
        t_crc = median3(timed(lambda: L.blissgpu_flac_crc16_device(
            ctx._h, C.c_void_p(d_bytes.data_ptr()), host.size - 16, big.ctypes.data_as(u64p), len(big), C.c_void_p(d_st.data_ptr()),
            C.c_void_p(d_end.data_ptr()), C.c_void_p(d_ok.data_ptr()))))[0]
        assert int((d_ok != 1).sum()) == 0
        res["c_kernels"][name] = {"frames": len(big), "compressed_MB": reps * b.size / 1e6, "decode_ms": t_dec * 1e3, "crc_ms": t_crc * 1e3,
                                  "crc_over_decode": t_crc / t_dec, "crc_GB_per_s": reps * b.size / t_crc / 1e9}
        # one song, one lane
        info1 = info.copy()
        t_md5 = median3(timed(lambda: L.blissgpu_flac_md5_device(ctx._h, C.c_void_p(d_pcm.data_ptr()), info1.ctypes.data_as(u64p),
                                                                 C.c_void_p(d_md5.data_ptr()))))[0]
        assert d_md5.cpu().numpy().tobytes() == info[8:10].tobytes(), name
        msg = total * ch * ((bps + 7) // 8)
        res["d_md5_lane"][name] = {"message_MB": msg / 1e6, "ms": t_md5 * 1e3, "MB_per_s_per_lane": msg / t_md5 / 1e6}
    rate = statistics.mean(v["MB_per_s_per_lane"] for v in res["d_md5_lane"].values())
    res["d_md5_three_minute_16bit_stereo_seconds_EXTRAPOLATED"] = 180 * 44100 * 2 * 2 / 1e6 / rate
    finish(res, args)


def finish(res, args):
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
