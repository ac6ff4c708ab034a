"""EBU R 128 loudness on the device (blissgpu_loudness_batch) against what a user had before it: a CPU scanner.

  device    `songs` three-minute stereo 16-bit songs at 44 100 Hz (seeded noise under a slow envelope, 16 different buffers handed
            in over and over: the call uploads every song's PCM, whatever its address) through loudness_batch -- the wall time
            of the host-pointer call, which uploads the PCM in its native format from pageable memory, and the HIP-event times of
            loud_energy_kernel, loud_peak_kernel and loud_fold_kernel from the context profiler: the kernels alone, PCM on the
            device.  Medians of `reps` after one warm-up.
  baseline  the same contract on the CPU: scipy.signal.sosfilt over each whole channel, numpy for the sub-block energies, the
            blocks, the gates, the range and the 4 x 49-tap interpolator -- ONE thread (the figure states it, and how many the
            machine would offer), `cpu_songs` songs measured and priced linearly for all of them: the figure says so.  Its
            loudness must agree with the device's.

    python tests/tools/loudness_bench.py [--songs 1024] [--seconds 180] [--reps 3] [--cpu-songs 2] [--out profiles/loudness_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
RATE, DISTINCT = 44100, 16


def cpu_loudness(bliss, a, rate, coef, h):
    """one song on the CPU: (lufs, range_lu, sample_peak, true_peak)"""
    from scipy.signal import sosfilt

    x = a.astype(np.float64) / 32768.0
    H = (rate + 5) // 10
    n_sub = x.shape[0] // H
    sos = np.array([[coef[0], coef[1], coef[2], 1.0, coef[3], coef[4]], [coef[5], coef[6], coef[7], 1.0, coef[8], coef[9]]])
    z = np.stack([(sosfilt(sos, x[:n_sub * H, c]).reshape(n_sub, H) ** 2).sum(axis=1) for c in range(x.shape[1])])
    four = np.lib.stride_tricks.sliding_window_view(z, 4, axis=1).sum(axis=2).sum(axis=0) / (4.0 * H)
    thirty = np.lib.stride_tricks.sliding_window_view(z, 30, axis=1).sum(axis=2).sum(axis=0) / (30.0 * H)
    lufs = bliss.loudness_gate(four)[1]  # (the gates are a few thousand operations: the library's device-free ones)
    lra = bliss.loudness_range(thirty)[0]
    tp = 0.0
    for c in range(x.shape[1]):
        for p in range(4):
            tp = max(tp, float(np.abs(np.convolve(x[:, c], h[p::4], mode="full")[6:6 + x.shape[0]]).max()))
    return lufs, lra, float(np.abs(x).max()), tp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=1024)
    ap.add_argument("--seconds", type=int, default=180)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-songs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loudness_bench.json"))
    args = ap.parse_args()
    import ctypes as C

    import torch

    import bliss_rs_amd as bliss
    from bliss_rs_amd import _ffi

    assert torch.cuda.is_available(), "loudness_bench measures on the GPU: there is no CPU path"
    ctx = bliss.Context.default()  # the host-pointer forms run on it

    def timed(f):
        ctx.synchronize()
        t0 = time.perf_counter()
        r = f()
        ctx.synchronize()
        return time.perf_counter() - t0, r

    n = args.seconds * RATE
    rng = np.random.default_rng(1)
    envelope = 0.05 + 0.25 * (0.5 + 0.5 * np.sin(2.0 * np.pi * np.arange(n + DISTINCT * 997) / (20.0 * RATE)))[:, None]
    base = np.round(32767.0 * np.clip(envelope * rng.standard_normal((n + DISTINCT * 997, 2)), -1.0, 1.0)).astype(np.int16)
    distinct = [base[i * 997:i * 997 + n] for i in range(DISTINCT)]
    songs = [distinct[i % DISTINCT] for i in range(args.songs)]
    header = open(os.path.join(ROOT, "include", "blissgpu.h")).read()
    out = {"device": torch.cuda.get_device_name(0), "library": os.path.basename(bliss.LIB_PATH), "songs": args.songs, "seconds": args.seconds,
           "rate": RATE, "channels": 2, "format": "s16", "reps": args.reps,
           "segment_in_this_tree": int(header.split("#define BLISSGPU_LOUDNESS_SEGMENT")[1].split()[0])}

    new = lambda: bliss.loudness_batch(songs, RATE)  # noqa: E731
    got = new()  # warm-up
    print("warm-up done", flush=True)
    walls = [timed(new)[0] for _ in range(args.reps)]
    ctx.synchronize()
    ctx.profile_enable(True)
    ctx.profile_reset()
    new()
    ctx.synchronize()
    prof = {name: [round(v[0], 4), int(v[1])] for name, v in ctx.profile().items() if v[1]}
    ctx.profile_enable(False)
    kernels_ms = sum(prof[k][0] for k in ("loud_energy_kernel", "loud_peak_kernel", "loud_fold_kernel"))
    samples = args.songs * n * 2
    wall_ms = 1e3 * statistics.median(walls)
    out["device_call"] = {"wall_ms": round(wall_ms, 3), "wall_ms_all": [round(1e3 * t, 3) for t in walls], "kernel_ms": prof,
                          "kernels_ms": round(kernels_ms, 3), "samples": samples,
                          "energy_gsamples_per_s": round(samples / prof["loud_energy_kernel"][0] / 1e6, 2),
                          "peak_gsamples_per_s": round(samples / prof["loud_peak_kernel"][0] / 1e6, 2),
                          "pcm_gib_uploaded": round(samples * 2 / 2 ** 30, 3), "share_of_wall_outside_the_kernels": round(1.0 - kernels_ms / wall_ms, 4),
                          "audio_hours_per_wall_second": round(args.songs * args.seconds / 3600.0 / (wall_ms / 1e3), 2)}
    print(json.dumps(out["device_call"]), flush=True)

    if args.cpu_songs:
        coef, factor, h = np.zeros(10), C.c_uint32(0), np.zeros(49)
        _ffi.call("blissgpu_loudness_kweighting", RATE, coef.ctypes.data_as(C.POINTER(C.c_double)))
        _ffi.call("blissgpu_true_peak_filter", RATE, C.byref(factor), h.ctypes.data_as(C.POINTER(C.c_double)))
        torch.set_num_threads(1)
        k = min(args.cpu_songs, args.songs)
        t0 = time.perf_counter()
        ref = [cpu_loudness(bliss, songs[i], RATE, coef, h) for i in range(k)]
        cpu_s = time.perf_counter() - t0
        worst = max(max(abs(r[0] - g.lufs), abs(r[1] - g.range_lu), abs(r[2] - g.sample_peak), abs(r[3] - g.true_peak)) for r, g in zip(ref, got))
        priced = cpu_s / k * args.songs
        out["cpu_baseline"] = {"what": "scipy.signal.sosfilt + numpy, the same contract", "threads": 1, "cpus_of_the_machine": os.cpu_count(),
                               "songs_measured": k, "seconds_measured": round(cpu_s, 3),
                               "seconds_priced_for_all_songs_not_measured": round(priced, 1),
                               "priced_over_device_wall": round(priced / (wall_ms / 1e3), 1),
                               "priced_over_device_wall_if_16_threads_scaled_perfectly": round(priced / 16.0 / (wall_ms / 1e3), 2),
                               "worst_difference_from_the_device": worst}
        print(json.dumps(out["cpu_baseline"]), flush=True)
        assert worst < 1e-6, worst
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
