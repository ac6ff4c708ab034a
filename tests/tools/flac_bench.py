#!/usr/bin/env python3
"""FLAC on the device against the host feed of decoded PCM: python tests/tools/flac_bench.py [--songs 4096] [--json out.json]

A batch of N "songs" from the bytes of tests/golden/s32_stereo_44_1_kHz.flac and testcue.flac, alternating (real encoder
output).  Each figure is the median of 3 runs after a warm-up:
  (a) blissgpu_analyze_batch_decoded on the same songs' decoded PCM in pageable host memory -- what a host has once its CPU
      decoder is finished, the decoder's own time left out
  (b) blissgpu_analyze_batch_flac on the compressed bytes
  (c) flac_decode_kernel alone (HIP events around blissgpu_flac_decode_device), samples/s over all channels
  (d) the host's frame indexing (fast mode), per song, one thread
  (e) the plain upload of the compressed bytes alone (pageable memory, one copy per song)
"""
import argparse
import ctypes as C
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
    return statistics.median(fn() for _ in range(3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=4096)
    ap.add_argument("--json", default="")
    ap.add_argument("--only-a", action="store_true", help="(a) alone: runs on a build without the FLAC entry points, such as the parent commit")
    args = ap.parse_args()
    import torch

    import bliss_rs_amd as bliss
    from bliss_rs_amd import _ffi
    from conftest import decoded_audio

    L = _ffi.lib()
    u64p = C.POINTER(C.c_uint64)
    names = ["s32_stereo_44_1_kHz.flac", "testcue.flac"]
    blobs = [np.fromfile(os.path.join(ROOT, "tests", "golden", n), np.uint8) for n in names]
    pcm = [np.ascontiguousarray(decoded_audio(n)[0]) for n in names]
    n = args.songs
    d = 23
    out = np.empty((n, d), np.float32)
    status = np.zeros(n, np.int32)
    stp = status.ctypes.data_as(C.POINTER(C.c_int32))

    songs = (_ffi.DecodedSong * n)()
    for i in range(n):
        a = pcm[i % 2]
        songs[i] = _ffi.DecodedSong(a.ctypes.data, a.shape[0], 44100, a.shape[1], _ffi.SAMPLE_S32 if a.dtype == np.int32 else _ffi.SAMPLE_S16)
    pcm_bytes = sum(pcm[i % 2].nbytes for i in range(n))

    def run_a():
        t0 = time.perf_counter()
        _ffi.check(L.blissgpu_analyze_batch_decoded(songs, n, 2, out.ctypes.data, stp))
        return time.perf_counter() - t0

    t_a = median3(run_a)
    rows_a = out.copy()
    if args.only_a:
        line = json.dumps({"songs": n, "pcm_GB": pcm_bytes / 1e9, "a_decoded_songs_per_s": n / t_a, "a_seconds": t_a, "a_GB_per_s": pcm_bytes / t_a / 1e9})
        print(line)
        if args.json:
            open(args.json, "w").write(line + "\n")
        return

    ptrs = (C.c_void_p * n)(*[blobs[i % 2].ctypes.data for i in range(n)])
    sizes = np.array([blobs[i % 2].size for i in range(n)], np.uint64)
    flac_bytes = int(sizes.sum())

    def run_b():
        t0 = time.perf_counter()
        _ffi.check(L.blissgpu_analyze_batch_flac(ptrs, sizes.ctypes.data_as(u64p), n, 2, out.ctypes.data, stp))
        return time.perf_counter() - t0

    t_b = median3(run_b)
    same = bool(np.array_equal(rows_a.view(np.uint32), out.view(np.uint32)))

    # (d) indexing, and the tables (c) needs
    tables, infos = [], []
    t_index = []
    for b in blobs:
        info = np.zeros(_ffi.FLAC_INFO_WORDS, np.uint64)
        nf = C.c_uint64(0)
        L.blissgpu_flac_index(C.c_void_p(b.ctypes.data), b.size, 0, info.ctypes.data_as(u64p), None, 0, C.byref(nf))
        tab = np.zeros((nf.value, 4), np.uint64)

        def index_once():
            t0 = time.perf_counter()
            L.blissgpu_flac_index(C.c_void_p(b.ctypes.data), b.size, 0, info.ctypes.data_as(u64p), tab.ctypes.data_as(u64p), nf.value, C.byref(nf))
            return time.perf_counter() - t0

        t_index.append(median3(index_once))
        tables.append(tab)
        infos.append(info)

    # (c) the decode kernel alone: one file per launch is too small to say anything, so a file is repeated inside ONE table
    ctx = bliss.Context(0)
    kernel = {}
    for name, b, tab, info in zip(names, blobs, tables, infos):
        reps = max(1, min(n // 2, 512))
        stride = (b.size + 16 + 15) // 16 * 16
        host = np.zeros(reps * stride + 16, np.uint8)
        big = np.zeros((reps * len(tab), 4), np.uint64)
        total, ch = int(info[3]), int(info[1])
        for r in range(reps):
            host[r * stride:r * stride + b.size] = b
            big[r * len(tab):(r + 1) * len(tab)] = tab
            big[r * len(tab):(r + 1) * len(tab), 0] += np.uint64(r * stride)
            big[r * len(tab):(r + 1) * len(tab), 2] += np.uint64(r * total)
        # (a fixed-block-size header does not code its position, so the repeated frames decode wherever the table puts them)
        info2 = info.copy()
        info2[3] = reps * total
        d_bytes = torch.from_numpy(host).cuda()
        d_pcm = torch.zeros((reps * total, ch), dtype=torch.int32 if int(info[2]) > 16 else torch.int16, device="cuda")
        d_st = torch.zeros(len(big), dtype=torch.int32, device="cuda")
        d_end = torch.zeros(len(big), dtype=torch.int64, device="cuda")

        def launch():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ctx._pre()   # (the context's stream waits for e0's stream and hands back to it: the events bracket the launch)
            _ffi.check(L.blissgpu_flac_decode_device(ctx._h, C.c_void_p(d_bytes.data_ptr()), host.size - 16, big.ctypes.data_as(u64p), len(big),
                                                     info2.ctypes.data_as(u64p), C.c_void_p(d_pcm.data_ptr()), C.c_void_p(d_st.data_ptr()),
                                                     C.c_void_p(d_end.data_ptr())))
            ctx._post()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3

        t = median3(launch)
        assert int(d_st.abs().sum()) == 0
        kernel[name] = {"frames": len(big), "ms": t * 1e3, "samples_per_s": reps * total * ch / t}

    # (e) what the plain upload of the compressed bytes costs: pageable host memory -> device, one copy per song
    dst = torch.empty(int(sizes.max()) * 2, dtype=torch.uint8, device="cuda")
    tblobs = [torch.from_numpy(b) for b in blobs]

    def upload():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            dst[:tblobs[i % 2].numel()].copy_(tblobs[i % 2], non_blocking=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    t_up = median3(upload)

    res = {
        "songs": n, "pcm_GB": pcm_bytes / 1e9, "flac_GB": flac_bytes / 1e9, "bytes_ratio": flac_bytes / pcm_bytes,
        "a_decoded_songs_per_s": n / t_a, "a_seconds": t_a, "a_GB_per_s": pcm_bytes / t_a / 1e9,
        "b_flac_songs_per_s": n / t_b, "b_seconds": t_b, "b_rows_equal_a": same,
        "c_decode_kernel": kernel,
        "d_index_us_per_song": {nm: t * 1e6 for nm, t in zip(names, t_index)},
        "e_pageable_upload_seconds": t_up, "e_pageable_upload_GB_per_s": flac_bytes / t_up / 1e9,
        "slow_songs": bliss.Context.default().flac_slow_songs(),
    }
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
