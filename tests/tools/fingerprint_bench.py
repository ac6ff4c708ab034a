"""Acoustic fingerprints on the device (blissgpu_fingerprint_batch / blissgpu_fingerprint_match) against what a
user had before them: torch on the same GPU evaluating the same contract.  Same process, alternating, medians of `reps` after one
warm-up of each.

  extraction  `songs` three-minute songs (seeded noise, every song its own rotation of one buffer) through fingerprint_batch --
              wall time of the host-pointer call, which uploads the PCM from pageable memory, and the HIP-event times of
              fp_bands_kernel and fp_bits_kernel from the context profiler -- against torch.stft (n_fft 8192, hop 512, the project's
              Hann table, no centring) in f32, the band sums and differences in f64, the words packed; the torch route is timed
              with the PCM already on the device, song by song, and its share of bits that differ from the device's is recorded
              (its FFT is another f32 FFT: a few bits near m = 0 differ).
  matching    `pairs` random pairs of `fps` random three-minute fingerprints at the default offsets (+-430, 256 positions)
              through playlist.fingerprint_match -- wall time and the kernels' times -- against a torch loop over the offsets:
              XOR of the shifted slices, popcount by a byte table, the zero mask, the exact comparison in int64, the contract's
              tie rule.  The torch loop runs `torch_pairs` of the pairs (its results must equal the device's) and is priced
              linearly for all of them: the figure says so.

    python tests/tools/fingerprint_bench.py [--songs 1024] [--pairs 100000] [--torch-pairs 2048] [--reps 3] [--out profiles/fingerprint_bench.json]
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
SR, W, HOP = 22050, 8192, 512
EDGES = [111, 118, 125, 132, 140, 149, 157, 167, 177, 187, 198, 210, 222, 235, 249, 264, 280, 296, 314, 332, 352, 373, 395, 418, 443, 469,
         497, 526, 557, 590, 625, 662, 702, 743]


def hann_f32():
    k = np.arange(W, dtype=np.float32)
    arg = np.float32(2.0) * k * np.float32(np.pi) / np.float32(W)
    return (np.float32(0.5) - np.float32(0.5) * np.cos(arg.astype(np.float64)).astype(np.float32)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--songs", type=int, default=1024)
    ap.add_argument("--seconds", type=int, default=180)
    ap.add_argument("--fps", type=int, default=1024)
    ap.add_argument("--pairs", type=int, default=100000)
    ap.add_argument("--torch-pairs", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fingerprint_bench.json"))
    args = ap.parse_args()
    import torch

    import bliss_rs_amd as bliss

    assert torch.cuda.is_available(), "fingerprint_bench measures on the GPU: there is no CPU path"
    P = bliss.playlist
    ctx = bliss.Context.default()  # the host-pointer forms run on it
    dev = torch.device("cuda")

    def sync():
        ctx.synchronize()
        torch.cuda.synchronize()

    def timed(f):
        sync()
        t0 = time.perf_counter()
        r = f()
        sync()
        return time.perf_counter() - t0, r

    def profiled(f):
        sync()
        ctx.profile_enable(True)
        ctx.profile_reset()
        r = f()
        sync()
        prof = {name: [round(v[0], 4), int(v[1])] for name, v in ctx.profile().items() if v[1]}
        ctx.profile_enable(False)
        return prof, r

    def ms(ts):
        return round(1e3 * statistics.median(ts), 3)

    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps}

    # ---- extraction ----
    if args.songs:
        n = args.seconds * SR
        base = (0.3 * np.random.default_rng(1).standard_normal(n + args.songs * 997)).astype(np.float32)
        songs = [base[i * 997:i * 997 + n] for i in range(args.songs)]
        window = torch.from_numpy(hann_f32()).to(dev)
        band = torch.zeros((EDGES[-1] - EDGES[0], 33), dtype=torch.float64, device=dev)
        for b in range(33):
            band[EDGES[b] - EDGES[0]:EDGES[b + 1] - EDGES[0], b] = 1.0
        weights = (2 ** torch.arange(32, dtype=torch.int64, device=dev))[None, :]
        d_songs = [torch.from_numpy(np.ascontiguousarray(s)).to(dev) for s in songs[:min(args.songs, 64)]]

        def torch_words(x):
            X = torch.stft(x, W, HOP, window=window, center=False, return_complex=True)[EDGES[0]:EDGES[-1]].T  # [frames, 632]
            E = (X.real.double() ** 2 + X.imag.double() ** 2) @ band
            d = E[:, :-1] - E[:, 1:]
            return (((d[1:] - d[:-1]) > 0).long() * weights).sum(dim=1)

        def torch_all():
            return [torch_words(d_songs[i % len(d_songs)]) for i in range(args.songs)]

        new = lambda: bliss.fingerprint_batch(songs)  # noqa: E731
        got, ref = new(), torch_all()  # warm-up of both
        print("extraction: warm-up done", flush=True)
        t_new, t_ref = [], []
        for _ in range(args.reps):
            t_new.append(timed(new)[0])
            t_ref.append(timed(torch_all)[0])
        prof = profiled(new)[0]
        differ = np.mean([(np.unpackbits((got[i] ^ ref[i].cpu().numpy().astype(np.uint32)).view(np.uint8))).mean() for i in range(len(d_songs))])
        frames = args.songs * ((n - W) // HOP + 1)
        kernels_ms = prof["fp_bands_kernel"][0] + prof["fp_bits_kernel"][0]
        out["extraction"] = {"songs": args.songs, "seconds": args.seconds, "frames": frames, "wall_ms": ms(t_new), "wall_ms_all": [round(1e3 * t, 3) for t in t_new],
                             "wall_ms_torch_pcm_on_device": ms(t_ref), "wall_ms_torch_all": [round(1e3 * t, 3) for t in t_ref], "kernel_ms": prof,
                             "kernels_ms": round(kernels_ms, 3), "frames_per_s_kernels": round(frames / kernels_ms * 1e3),
                             "pcm_gib_uploaded": round(args.songs * n * 4 / 2 ** 30, 3), "share_of_bits_differing_from_torch": float(differ)}
        print(json.dumps(out["extraction"]), flush=True)
        del d_songs, songs, base

    # ---- matching ----
    if args.pairs:
        rng = np.random.default_rng(2)
        L = (args.seconds * SR - W) // HOP
        fps = [rng.integers(1, 2 ** 32, L, dtype=np.uint64).astype(np.uint32) for _ in range(args.fps)]
        pairs = rng.integers(0, args.fps, (args.pairs, 2))
        O, MIN = P.FINGERPRINT_MAX_OFFSET, P.FINGERPRINT_MIN_OVERLAP
        F = torch.from_numpy(np.stack(fps).view(np.int32)).to(dev)
        table = torch.tensor([bin(i).count("1") for i in range(256)], dtype=torch.int32, device=dev)
        tp = min(args.torch_pairs, args.pairs)
        pt = torch.from_numpy(pairs[:tp]).to(dev)

        def torch_match():
            a, b = F[pt[:, 0]], F[pt[:, 1]]
            best_e = torch.zeros(tp, dtype=torch.int64, device=dev)
            best_v = torch.zeros_like(best_e)  # 0: nothing yet
            best_o = torch.zeros_like(best_e)
            for o in sorted(range(-O, O + 1), key=lambda o: (abs(o), o)):
                lo, hi = max(0, -o), min(L, L - o)
                av, bv = a[:, lo:hi], b[:, lo + o:hi + o]
                valid = (av != 0) & (bv != 0)
                pop = table[(av ^ bv).view(torch.uint8).int()].view(tp, hi - lo, 4).sum(dim=2)
                e = (pop * valid).sum(dim=1, dtype=torch.int64)
                v = valid.sum(dim=1, dtype=torch.int64)
                better = (v >= MIN) & ((best_v == 0) | (e * best_v < best_e * v))
                best_e, best_v, best_o = torch.where(better, e, best_e), torch.where(better, v, best_v), torch.where(better, o, best_o)
            return best_o, best_e, 32 * best_v

        new = lambda: P.fingerprint_match(fps, pairs, O, MIN)  # noqa: E731
        got, ref = new(), torch_match()  # warm-up of both
        print("matching: warm-up done", flush=True)
        same = all(np.array_equal(g[:tp].astype(np.int64), r.cpu().numpy()) for g, r in zip(got, ref))
        t_new, t_ref = [], []
        for _ in range(args.reps):
            t_new.append(timed(new)[0])
            t_ref.append(timed(torch_match)[0])
        prof = profiled(new)[0]
        steps = args.pairs * (2 * O + 1) * L  # (pair, offset, position) triples, the few an offset shifts out included
        out["matching"] = {"fingerprints": args.fps, "words": int(L), "pairs": args.pairs, "max_offset": O, "min_overlap": MIN, "wall_ms": ms(t_new),
                           "wall_ms_all": [round(1e3 * t, 3) for t in t_new], "kernel_ms": prof,
                           "word_compares_per_s_kernel": round(steps / prof["fp_match_kernel"][0] * 1e3), "torch_pairs": tp,
                           "torch_wall_ms_for_torch_pairs": ms(t_ref), "torch_wall_ms_all": [round(1e3 * t, 3) for t in t_ref],
                           "torch_ms_priced_for_all_pairs_not_measured": round(ms(t_ref) * args.pairs / tp, 1),
                           "torch_results_equal_the_devices": bool(same)}
        print(json.dumps(out["matching"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
