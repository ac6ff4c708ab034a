// kernels_tempo.hip -- aubio-style tempo on the device (compiled with -ffp-contract=off so every
// f32 operation rounds exactly like the reference's scalar Rust).
//
//   onset_kernel : PeakPicker threshold (src/aubio.rs:733-768, 661-685, 482-554): a pure function of
//                  the last 7 SpecFlux values, so one thread per tempo frame.
//   beat_acf_kernel   : the state-independent half of BeatTracking::do_ (src/aubio.rs:966-1003): the
//                  autocorrelation of every run's detection-function frame, its comb filterbank sums
//                  for both time signatures, the Rayleigh-weighted period and get_timesig (:864-907)
//                  -- one workgroup per eight consecutive runs of a song, ~124 k runs for 1024 three-minute songs.
//   beat_track_kernel : the sequential half: checkstate (:1096-1227), beat phase (:1025-1054),
//                  Tempo::do_'s beat / silence test (:1378-1443), get_bpm and BPMDesc's median
//                  (src/temporal.rs:50-77).  The chain (gp/rp1/rp2/counter/flagstep/timesig/lastbeat/
//                  gwv/phwv) is walked by ONE wavefront per song with no workgroup barrier: its inputs are
//                  prefetched a run ahead, so a run costs a few microseconds and the kernel holds 1/16 of
//                  the registers the former one-workgroup-per-song tracker did.
#include "device_utils.hpp"
#include "internal.hpp"

namespace bg {

// correctly rounded f32 exp via f64 (glibc's expf, which the reference links, is correctly rounded
// in all but vanishingly rare cases)
__device__ __forceinline__ float exp_f32(float x) { return (float)exp((double)x); }

// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void onset_kernel(const SongDesc* __restrict__ songs,
                                                    const float* __restrict__ flux,
                                                    float* __restrict__ thresholded) {
    const SongDesc sd = songs[blockIdx.y];
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (!sd.ok || t >= sd.n_b) return;
    const float* f = flux + sd.b_off;
    // onset_keep after pushing frame t: [f[t-6] .. f[t]], zeros before the song starts
    float p[7], tmp[7];
#pragma unroll
    for (int i = 0; i < 7; i++) {
        const long idx = (long)t - 6 + i;
        p[i] = idx >= 0 ? f[idx] : 0.0f;
    }
    // Biquad::do_filtfilt (state reset before each pass); a2 = 0
    const float b0 = 0.1599879f, b1 = 0.31997577f, b2 = 0.1599879f, a1 = 0.23484048f, a2 = 0.0f;
    float x1 = 0.f, x2 = 0.f, y1 = 0.f, y2 = 0.f;
#pragma unroll
    for (int i = 0; i < 7; i++) {
        const float x0 = p[i];
        const float y0 = b0 * x0 + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2;
        x2 = x1; x1 = x0; y2 = y1; y1 = y0;
        p[i] = y0;
    }
#pragma unroll
    for (int i = 0; i < 7; i++) tmp[6 - i] = p[i];
    x1 = x2 = y1 = y2 = 0.f;
#pragma unroll
    for (int i = 0; i < 7; i++) {
        const float x0 = tmp[i];
        const float y0 = b0 * x0 + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2;
        x2 = x1; x1 = x0; y2 = y1; y1 = y0;
        tmp[i] = y0;
    }
#pragma unroll
    for (int i = 0; i < 7; i++) p[i] = tmp[6 - i];
    // vec_mean (sequential) and vec_median (element (n-1)/2 = 3 of the sorted 7)
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < 7; i++) sum += p[i];
    const float mean = sum / 7.0f;
    const float p5 = p[5];
#pragma unroll
    for (int i = 0; i < 7; i++)
#pragma unroll
        for (int j = 0; j + 1 < 7 - i; j++) {
            const float lo = fminf(p[j], p[j + 1]), hi = fmaxf(p[j], p[j + 1]);
            p[j] = lo; p[j + 1] = hi;
        }
    const float median = p[3];
    thresholded[sd.b_off + t] = p5 - median - mean * 0.3f;  // threshold 0.3 (src/aubio.rs:1347)
}

void launch_onset(const Batch& b, const Workspace& w, hipStream_t st) {
    // grid.x sized for the longest song is computed by the caller through total_b / n_songs upper bound
    if (b.n_songs == 0 || b.total_b == 0) return;
    // the host passes the maximum n_b in tiles_e's sibling: recomputed here from total_b would be wrong
    // for ragged batches, so Batch carries it in max_nb (see blissgpu.hip)
    hipLaunchKernelGGL(onset_kernel, dim3((uint32_t)((b.max_nb + 255) / 256), b.n_songs), dim3(256), 0, st, b.songs,
                       w.flux, w.thresholded);
}

// ------------------------------------------------------------------------------------------------
// vec_max_elem (src/aubio.rs:787-799): last index attaining the maximum, scanning with tmp = 0 (so a
// vector with no element >= 0 yields index 0).  One wavefront; element i = lane + 64 q is x[q].
// Returns (value, index) with value = -1 when no element is >= 0.
template <int Q>
__device__ __forceinline__ void wave_argmax_last(const float (&x)[Q], float* val, int* idx) {
    const int lane = lane_id();
    float best = -1.0f;  // "no candidate" marker: candidates are >= 0
    int bidx = 0;
#pragma unroll
    for (int q = 0; q < Q; q++) {
        if (x[q] >= 0.0f && x[q] >= best) { best = x[q]; bidx = lane + 64 * q; }  // index increases: keeps the last among equals
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(best, off, WAVE);
        const int oi = __shfl_xor(bidx, off, WAVE);
        if (ov > best || (ov == best && oi > bidx)) { best = ov; bidx = oi; }
    }
    *val = best;
    *idx = (best < 0.0f) ? 0 : bidx;
}

// vec_quadratic_peak_pos (src/aubio.rs:576-604)
__device__ __forceinline__ float quad_peak_pos(const float* x, int len, int pos) {
    if (pos == 0 || pos >= len - 1) return (float)pos;
    const float s0 = x[pos - 1], s1 = x[pos], s2 = x[pos + 1];
    return (float)pos + 0.5f * (s0 - s2) / (s0 - 2.0f * s1 + s2);
}

// get_timesig (src/aubio.rs:864-907), acflen = 512
__device__ float bt_timesig(const float* acf, long gp) {
    if (gp < 2) return 4;
    float three = 0.0f, four = 0.0f;
    const long acflen = BT_WINLEN;
    if (acflen > 6 * gp + 2) {
        for (long k = -2; k < 2; k++) { three += acf[3 * gp + k]; four += acf[4 * gp + k]; }
    } else {
        for (long k = -2; k < 2; k++) {
            const long i3 = 3 * gp + k, i6 = 6 * gp + k, i4 = 4 * gp + k, i2 = 2 * gp + k;
            if (i3 < acflen && i6 < acflen) three += acf[i3] + acf[i6];
            else if (i3 < acflen) three += acf[i3];
            if (i4 < acflen && i2 < acflen) four += acf[i4] + acf[i2];
            else if (i4 < acflen) four += acf[i4];
        }
    }
    return three > four ? 3 : 4;
}

// Per-run record written by beat_acf_kernel: everything BeatTracking::do_ derives from the run's frame alone.
//   [0, 128)   g3: unweighted comb sums for time signature 3 (the gwv path of checkstate, :1110-1124)
//   [128, 256) g4: the same for time signature 4
//   [256] rp3  [257] rp4 : Rayleigh-weighted period with numelem 3 / 4 (:987-1013)
//   [258] ts3  [259] ts4 : get_timesig(acf, rp3 / rp4), what checkstate would set when it locks onto that period
constexpr int BT_PRE_G3 = 0, BT_PRE_G4 = BT_LAGLEN, BT_PRE_RP3 = 256, BT_PRE_RP4 = 257, BT_PRE_TS3 = 258, BT_PRE_TS4 = 259;
static_assert(BT_PRE_STRIDE >= 260, "per-run record");

typedef float bt_f2 __attribute__((ext_vector_type(2)));

// A workgroup takes ACF_RUNS consecutive runs of one song; each of its four wavefronts takes one quarter of the lags of
// all of them (see beat_acf_kernel).  A run's frame lies in LDS at a pitch of ACF_PITCH floats: 512 values, then zeros up to
// the last index a lane reads (575 in df, 576 == df1[575]); 580 = 4 (mod 64) spreads the eight runs of a wavefront over
// the banks (a lane reads 16-byte pieces at a stride of 8 floats inside a run).  (Frame starts at 0, 4, 36, 32 mod 64 make
// every read conflict-free and buy nothing: the kernel waits for its multiply-adds, not for LDS.)
constexpr int ACF_RUNS = 8, ACF_PITCH = 580;
static_assert(ACF_PITCH >= BT_WINLEN + 65 && ACF_PITCH % 4 == 0, "zero padding behind a frame, 16-byte aligned frames");

// acc[k] += f[i] * (w[i + 2k], w[i + 2k + 1]) for 16 consecutive i: the eight lags (L .. L + 7) of one thread, w = frame + L.
// The packed multiply / add takes two lags per instruction; w1 is the same series one element on (a second copy in LDS),
// so that the odd steps' operand pairs also arrive in even-aligned register pairs (gfx950 takes 64-bit operands from
// aligned pairs only, and a copy per step costs more than the LDS read).  Eight lags per thread: 22 + 22 values and the
// 16 first factors feed 128 multiply-adds, and every sum is one of four independent chains.
__device__ __forceinline__ void acf_block16(bt_f2 (&acc)[4], const float* w, const float* w1, const float* f) {
    float r[24], r1[24], fv[16];
#pragma unroll
    for (int u = 0; u < 24; u++) { r[u] = w[u]; r1[u] = w1[u]; }
#pragma unroll
    for (int u = 0; u < 16; u++) fv[u] = f[u];
#pragma unroll
    for (int u = 0; u < 16; u += 2) {
        const bt_f2 fv0 = {fv[u], fv[u]}, fv1 = {fv[u + 1], fv[u + 1]};
#pragma unroll
        for (int k = 0; k < 4; k++) {  // step u: w[u .. u+7]
            const bt_f2 e = {r[u + 2 * k], r[u + 2 * k + 1]};
            acc[k] = acc[k] + fv0 * e;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {  // step u + 1: w[u+1 .. u+8]
            const bt_f2 o = {r1[u + 2 * k], r1[u + 2 * k + 1]};
            acc[k] = acc[k] + fv1 * o;
        }
    }
}

__global__ __launch_bounds__(256) void beat_acf_kernel(const SongDesc* __restrict__ songs,
                                                       const float* __restrict__ thresholded,
                                                       const float* __restrict__ rwv_tab,
                                                       float* __restrict__ pre_all) {
    // df[r]: the frame of run m0 + r, zeros behind it (the ACF loops read past the frame instead of predicating);
    // df1[r][j] = df[r][j + 1].  Once the autocorrelation is done the same memory holds acf[r][512] and acfout[r][2][128].
    __shared__ __attribute__((aligned(16))) float df[ACF_RUNS * ACF_PITCH];
    __shared__ __attribute__((aligned(16))) float df1[ACF_RUNS * ACF_PITCH];
    static_assert(ACF_PITCH >= BT_WINLEN && ACF_PITCH >= 2 * BT_LAGLEN, "acf / acfout live in a run's own frame");
    const uint32_t s = blockIdx.y;
    const long m0 = (long)blockIdx.x * ACF_RUNS;
    const SongDesc sd = songs[s];
    if (!sd.ok) return;
    const long n_b = sd.n_b;
    const long n_runs = (n_b >= BT_STEP) ? (n_b - BT_STEP) / BT_STEP + 1 : 0;
    if (m0 >= n_runs) return;  // uniform over the workgroup
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // in a scalar register: the loop bounds below depend on it
    const float* thr = thresholded + sd.b_off;

    // ---- dfframe for run m: s[128(m+1)-512+i], s[x] = 0 for x <= 0, thr[x-1] otherwise (Tempo::do_ :1389-1416); runs
    //      behind the song's last one get a frame of zeros (their results are never stored) ----
    {
        constexpr int per = ACF_RUNS * ACF_PITCH / 256 + 1;
        float v[per];
#pragma unroll
        for (int q = 0; q < per; q++) {  // all loads in flight together; the address is clamped instead of branching
            const int e = tid + 256 * q, r = e / ACF_PITCH, i = e - r * ACF_PITCH;
            const long m = m0 + r, xi = 128 * (m + 1) - 512 + i;
            const bool live = e < ACF_RUNS * ACF_PITCH && i < BT_WINLEN && m < n_runs && xi > 0;
            const float x = thr[live ? xi - 1 : 0];
            v[q] = live ? x : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < per; q++) {
            const int e = tid + 256 * q, r = e / ACF_PITCH, i = e - r * ACF_PITCH;
            if (e < ACF_RUNS * ACF_PITCH) {
                df[e] = v[q];
                if (i > 0) df1[e - 1] = v[q];
                if (i == ACF_PITCH - 1) df1[e] = 0.0f;
            }
        }
    }
    __syncthreads();
    // vec_autocorr (:819-828): acf[L] = (sum_{j=L}^{511} f[j-L] f[j]) / (512 - L), summed in j order.  Wavefront w owns the
    // lags [64 w, 64 w + 64) and [448 - 64 w, 512 - 64 w) -- a long and a short quarter -- of all eight runs: lane 8 r + g
    // has the lag octets (64 w + 8 g ..) and (504 - 64 w - 8 g ..) of run r and runs i = j - L over the eight lags of an
    // octet at once (packed multiply, packed add: two lags per instruction).  The loops run to bounds that are uniform over
    // the wavefront, 512 - 64 w and 64 (w + 1) steps (what its smallest lag of each kind needs; 576 together for every
    // wavefront, where one wavefront with all lags of a run would need 512 + 256), and read the zero padding behind the
    // frame instead of predicating (x + f * 0 == x exactly, so every sum is bit-identical to the reference's).  The first
    // factor f[i] differs between the runs of a wavefront, so it is an LDS read too (the same address for the 8 lanes of a run).
    const int r = lane >> 3, g = lane & 7;
    const int la = 64 * wave + 8 * g, lb = BT_WINLEN - 8 - 64 * wave - 8 * g;
    bt_f2 sa[4], sb[4];
    {
        const int na = BT_WINLEN - 64 * wave, nb = 64 * (wave + 1);
        const float* fr = df + r * ACF_PITCH;
        const float* fr1 = df1 + r * ACF_PITCH;
#pragma unroll
        for (int k = 0; k < 4; k++) { sa[k] = bt_f2{0.0f, 0.0f}; sb[k] = bt_f2{0.0f, 0.0f}; }
        for (int i = 0; i < na; i += 16) acf_block16(sa, fr + la + i, fr1 + la + i, fr + i);
        for (int i = 0; i < nb; i += 16) acf_block16(sb, fr + lb + i, fr1 + lb + i, fr + i);
    }
    __syncthreads();  // every frame has been read: its memory becomes the run's acf / acfout
    {
        float* acf = df + r * ACF_PITCH;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            acf[la + 2 * k] = sa[k].x / (float)(BT_WINLEN - la - 2 * k);
            acf[la + 2 * k + 1] = sa[k].y / (float)(BT_WINLEN - la - 2 * k - 1);
            acf[lb + 2 * k] = sb[k].x / (float)(BT_WINLEN - lb - 2 * k);
            acf[lb + 2 * k + 1] = sb[k].y / (float)(BT_WINLEN - lb - 2 * k - 1);
        }
    }
    __syncthreads();
    // From here a wavefront finishes two of the runs, one after the other (nothing below for a run behind the song's end).
    // shift-invariant comb filterbank (:987-1003): the sums run a = 1 .. numelem in order, so the numelem = 4 value is
    // the numelem = 3 value continued.  Rayleigh path: terms divided by 2a - 1, weighted by rwv; the unweighted sums
    // are what checkstate weights by its Gaussian (:1110-1124).
    for (int rr = 2 * wave; rr < 2 * wave + 2; rr++) {
        const long m = m0 + rr;
        if (m >= n_runs) break;  // uniform over the wavefront
        const float* acf = df + rr * ACF_PITCH;
        float* acfout = df1 + rr * ACF_PITCH;  // [2][BT_LAGLEN]
        float* pre = pre_all + ((size_t)(sd.b_off / BT_STEP) + s + (size_t)m) * BT_PRE_STRIDE;
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const int l = lane + 64 * half;
            float v3 = 0.0f, v4 = 0.0f, g3 = 0.0f, g4 = 0.0f;
            if (l >= 1 && l < BT_LAGLEN - 1) {
                float v = 0.0f, gs = 0.0f;
                for (int a = 1; a <= 4; a++) {
                    if (a == 4) { v3 = v; g3 = gs; }
                    for (int b = 1; b < 2 * a; b++) {
                        const int idx = l * a + b - 1;
                        if (idx < BT_WINLEN) {
                            v += acf[idx] / (2.0f * (float)a - 1.0f);
                            gs += acf[idx];
                        }
                    }
                }
                v4 = v; g4 = gs;
            }
            const float rw = rwv_tab[l];
            acfout[l] = v3 * rw;
            acfout[BT_LAGLEN + l] = v4 * rw;
            pre[BT_PRE_G3 + l] = g3;
            pre[BT_PRE_G4 + l] = g4;
        }
        // acfout[rr] is written and read by this wavefront alone; LDS operations of a wavefront complete in order
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int which = 0; which < 2; which++) {
            const float* ao = acfout + which * BT_LAGLEN;
            const float x[2] = {ao[lane], ao[lane + 64]};
            float best;
            int maxindex;
            wave_argmax_last(x, &best, &maxindex);
            if (lane == 0) {
                const int rayparam = 43;  // (60*22050/120/256) as u32
                const float rp = (maxindex > 0 && maxindex < BT_LAGLEN - 1) ? quad_peak_pos(ao, BT_LAGLEN, maxindex)
                                                                           : (float)rayparam;
                pre[BT_PRE_RP3 + which] = rp;
                pre[BT_PRE_TS3 + which] = bt_timesig(acf, (long)rp);
            }
        }
    }
}

struct BtShared {
    float dfrev[BT_WINLEN];
    float acfout[BT_LAGLEN];
    float phout[BT_LAGLEN + 1];  // [128] stays zero: phout is zero from the beat period on (bp < 128)
    float out[BT_STEP];
};

__global__ __launch_bounds__(64) void beat_track_kernel(const SongDesc* __restrict__ songs,
                                                        const float* __restrict__ thresholded,
                                                        const float* __restrict__ e256,
                                                        const float* __restrict__ dfwv_tab,
                                                        const float* __restrict__ pre_all,
                                                        float* __restrict__ run_bpm, uint32_t* __restrict__ run_cnt,
                                                        uint32_t runs_pitch, TempoState* __restrict__ tempo_out) {
    __shared__ BtShared sh;
    const uint32_t s = blockIdx.x;
    const SongDesc sd = songs[s];
    const int lane = threadIdx.x;
    if (!sd.ok) {
        if (lane == 0) { tempo_out[s].tempo = -1.0f; tempo_out[s].n_bpms = 0; }
        return;
    }
    const float* thr = thresholded + sd.b_off;
    const float* en = e256 + sd.e_off;
    const float* pre_song = pre_all + ((size_t)(sd.b_off / BT_STEP) + s) * BT_PRE_STRIDE;
    float* rbpm = run_bpm + (size_t)s * runs_pitch;
    uint32_t* rcnt = run_cnt + (size_t)s * runs_pitch;

    float dfwv[8];
#pragma unroll
    for (int q = 0; q < 8; q++) dfwv[q] = dfwv_tab[lane + 64 * q];
    float gwv[2] = {0.0f, 0.0f};
    if (lane == 0) sh.phout[BT_LAGLEN] = 0.0f;
    // scalar state: every lane carries the same values
    float gp_state = 0.0f, rp1 = 0.0f, rp2 = 0.0f, lastbeat = 0.0f;
    int counter = 0, flagstep = 0, timesig = 0;

    const float g_var = 3.901f;
    const long n_b = sd.n_b;
    long n_runs = (n_b >= BT_STEP) ? (n_b - BT_STEP) / BT_STEP + 1 : 0;  // runs happen at tempo frames 127 + 128 m
    if (n_runs > (long)runs_pitch) n_runs = (long)runs_pitch;

    // everything a run reads from memory is independent of the tracker's state: fetched one run ahead
    struct RunIn {
        float f[8];         // dfframe[lane + 64 q]
        float g3[2], g4[2];  // comb sums at lags lane, lane + 64
        float rp3, rp4, ts3, ts4;
        float e[2], e1[2];   // 256-sample energies of tempo frames 127 + 128 m + (lane, lane + 64) and the following block
    };
    auto fetch = [&](long m, RunIn& r) {
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const long xi = 128 * (m + 1) - 512 + lane + 64 * q;
            r.f[q] = (xi <= 0) ? 0.0f : thr[xi - 1];
        }
        const float* pre = pre_song + (size_t)m * BT_PRE_STRIDE;
#pragma unroll
        for (int q = 0; q < 2; q++) {
            r.g3[q] = pre[BT_PRE_G3 + lane + 64 * q];
            r.g4[q] = pre[BT_PRE_G4 + lane + 64 * q];
            const long t = 127 + 128 * m + lane + 64 * q;
            r.e[q] = t < n_b ? en[t] : 1.0f;
            r.e1[q] = t < n_b ? en[t + 1] : 1.0f;
        }
        r.rp3 = pre[BT_PRE_RP3]; r.rp4 = pre[BT_PRE_RP4]; r.ts3 = pre[BT_PRE_TS3]; r.ts4 = pre[BT_PRE_TS4];
    };
    RunIn cur, nxt;
    if (n_runs > 0) fetch(0, cur);

    for (long m = 0; m < n_runs; m++) {
        if (m + 1 < n_runs) fetch(m + 1, nxt);
        // dfrev = reverse(dfframe * dfwv) (:975-980)
#pragma unroll
        for (int q = 0; q < 8; q++) sh.dfrev[BT_WINLEN - 1 - (lane + 64 * q)] = cur.f[q] * dfwv[q];
        // the Rayleigh-weighted period for the current numelem (:983-1013)
        const float rp = (timesig == 3) ? cur.rp3 : cur.rp4;

        // ---- checkstate (:1096-1227) ----
        float gp = gp_state;
        if (gp > 0.0f) {  // uniform; implies timesig in {3, 4}
            const float x[2] = {(timesig == 3 ? cur.g3[0] : cur.g4[0]) * gwv[0], (timesig == 3 ? cur.g3[1] : cur.g4[1]) * gwv[1]};
            sh.acfout[lane] = x[0];
            sh.acfout[lane + 64] = x[1];
            float best;
            int maxindex;
            wave_argmax_last(x, &best, &maxindex);
            __syncthreads();
            gp = quad_peak_pos(sh.acfout, BT_LAGLEN, maxindex);
        } else {
            gp = 0.0f;
        }
        int flagconst = 0;
        if (counter == 0) {
            if (fabsf(gp - rp) > 2.0f * g_var) { flagstep = 1; counter = 3; }
            else flagstep = 0;
        }
        if (counter == 1 && flagstep == 1) {
            if (fabsf(2.0f * rp - rp1 - rp2) < g_var) { flagconst = 1; counter = 0; }
            else { flagconst = 0; counter = 2; }
        } else if (counter > 0) {
            counter -= 1;
        }
        rp2 = rp1;
        rp1 = rp;
        float bp;
        int phw_mode;  // 0 = flat, 1 = gaussian
        if (flagconst) {
            gp = rp;
            timesig = (int)((timesig == 3) ? cur.ts3 : cur.ts4);  // get_timesig(acf, gp) with gp = this run's rp
            bp = gp;
            phw_mode = 0;
        } else if (timesig > 0) {
            bp = gp;
            phw_mode = ((float)BT_STEP > lastbeat) ? 1 : 0;
        } else {
            bp = rp;
            phw_mode = 0;
        }
        const float bpw = bp;
        while (bp > 0.0f && bp < 25.0f) bp *= 2.0f;
        gp_state = gp;
        if (flagconst) {
#pragma unroll
            for (int q = 0; q < 2; q++) {
                const float diff = (float)(lane + 64 * q + 1) - gp;
                gwv[q] = exp_f32(-0.5f * diff * diff / (g_var * g_var));
            }
        }

        uint32_t nbeats = 0;
        if (bp != 0.0f) {  // uniform
            // beat phase (:1025-1054): phout[i] is non-zero only for i < bp (< 128), where phwv applies
            const int kmax = (int)floorf((float)BT_WINLEN / bp);
            __syncthreads();  // dfrev is complete
            float ph[2];
#pragma unroll
            for (int q = 0; q < 2; q++) {
                const int i = lane + 64 * q;
                float v = 0.0f;
                if ((float)i < bp) {
                    for (int k = 0; k < kmax; k++) {
                        const int idx = i + (int)floorf((bp * (float)k) + 0.5f);
                        if (idx < BT_WINLEN) v += sh.dfrev[idx];
                    }
                }
                float w = 1.0f;
                if (phw_mode == 1) {
                    const float diff = 1.0f + (float)i - (float)BT_STEP + lastbeat;
                    w = exp_f32(-0.5f * diff * diff / (bpw / 8.0f));
                }
                ph[q] = v * w;
                sh.phout[i] = ph[q];
            }
            float best;
            int maxindex;
            wave_argmax_last(ph, &best, &maxindex);
            // the frame's remaining entries (128..511) are zero: the last of them wins unless an earlier one is positive
            if (!(best > 0.0f)) maxindex = BT_WINLEN - 1;
            __syncthreads();
            float phase;
            if (maxindex >= BT_WINLEN - 1) phase = (float)BT_STEP - lastbeat;
            else phase = quad_peak_pos(sh.phout, BT_WINLEN, maxindex);  // maxindex < 128: reads at most phout[128] == 0
            phase += 1.0f;
            int i = 1;
            float beat = bp - phase;
            if (((float)BT_STEP - lastbeat - phase) < -0.40f * bp) beat += bp;
            while (beat + bp < 0.0f) beat += bp;
            if (beat >= 0.0f && i < BT_STEP) { if (lane == 0) sh.out[i] = beat; i++; }
            while (beat + bp <= (float)BT_STEP && i < BT_STEP) { beat += bp; if (lane == 0) sh.out[i] = beat; i++; }
            lastbeat = beat;
            nbeats = (uint32_t)i;
            __syncthreads();
        }

        // ---- frames 127+128m .. 127+128m+127 use out/bp of this run (Tempo::do_ :1418-1438) ----
        uint32_t hits = 0;
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int j = lane + 64 * q;  // blockpos
            const long t = 127 + 128 * m + j;
            float tempo = 0.0f;
            if (t < n_b) {
                for (uint32_t i = 1; i < nbeats; i++) {
                    const float beat_pos = sh.out[i];
                    if (j == (int)floorf(beat_pos)) {
                        tempo = beat_pos - floorf(beat_pos);
                        // is_silence over the 512-sample window analyze() passed: x[256t, 256t+512),
                        // i.e. the 256-sample energy blocks t and t+1
                        const float level = (cur.e[q] + cur.e1[q]) / 512.0f;
                        if (10.0f * log10f(level) < -90.0f) tempo = 0.0f;
                    }
                }
            }
            hits += (uint32_t)__popcll(__ballot(tempo > 0.0f));
        }
        if (lane == 0) {
            // BeatTracking::get_bpm (:1231-1239)
            float bpm = 0.0f;
            if (bp != 0.0f) {
                const float period_samples = (float)HOP_B * bp;
                const float period_s = period_samples / (float)SAMPLE_RATE;
                bpm = 60.0f / period_s;
            }
            rbpm[m] = bpm;
            rcnt[m] = hits;
        }
        __syncthreads();  // out / dfrev / phout are rewritten by the next run
        cur = nxt;
    }
    __threadfence_block();
    __syncthreads();

    // ---- BPMDesc::get_value (src/temporal.rs:66-77): Midpoint median of the pushed bpms ----
    const long runs = n_runs;
    uint32_t tot = 0;
    for (long m = lane; m < runs; m += WAVE) tot += rcnt[m];
    const uint32_t total = wave_sum(tot);
    if (total == 0) {
        if (lane == 0) { tempo_out[s].tempo = -1.0f; tempo_out[s].n_bpms = 0; }
        return;
    }
    const uint32_t r_lo = (total - 1) / 2, r_hi = (total - 1) - r_lo == r_lo ? r_lo : r_lo + 1;
    // equal values yield the same number, so "any lane that holds the order statistic" is well defined
    float lo = 0.0f, hi = 0.0f;
    bool has_lo = false, has_hi = false;
    for (long m = lane; m < runs; m += WAVE) {
        const uint32_t c = rcnt[m];
        if (c == 0) continue;
        const float v = rbpm[m];
        uint32_t less = 0, leq = 0;
        for (long q = 0; q < runs; q++) {
            const uint32_t cq = rcnt[q];
            if (cq == 0) continue;
            const float vq = rbpm[q];
            if (vq < v) less += cq;
            if (vq <= v) leq += cq;
        }
        if (less <= r_lo && r_lo < leq) { lo = v; has_lo = true; }
        if (less <= r_hi && r_hi < leq) { hi = v; has_hi = true; }
    }
    const uint64_t m_lo = __ballot(has_lo), m_hi = __ballot(has_hi);
    const float s_lo = m_lo ? __shfl(lo, __ffsll((unsigned long long)m_lo) - 1, WAVE) : 0.0f;
    const float s_hi = m_hi ? __shfl(hi, __ffsll((unsigned long long)m_hi) - 1, WAVE) : 0.0f;
    if (lane == 0) {
        const float median = s_lo + (s_hi - s_lo) / 2.0f;
        tempo_out[s].tempo = 2.0f * (median - 0.0f) / (206.0f - 0.0f) - 1.0f;
        tempo_out[s].n_bpms = total;
    }
}

void launch_beat_acf(const Batch& b, const Workspace& w, const DeviceTables& t, hipStream_t st) {
    if (b.n_songs == 0) return;
    const uint32_t max_runs = b.max_nb >= (uint32_t)BT_STEP ? (b.max_nb - BT_STEP) / BT_STEP + 1 : 0;
    if (max_runs > 0)
        hipLaunchKernelGGL(beat_acf_kernel, dim3((max_runs + ACF_RUNS - 1) / ACF_RUNS, b.n_songs), dim3(256), 0, st, b.songs,
                           w.thresholded, t.bt_rwv, w.bt_pre);
}

void launch_beat_track(const Batch& b, const Workspace& w, const DeviceTables& t, hipStream_t st) {
    if (b.n_songs == 0) return;
    hipLaunchKernelGGL(beat_track_kernel, dim3(b.n_songs), dim3(64), 0, st, b.songs, w.thresholded, w.e256, t.bt_dfwv,
                       w.bt_pre, w.run_bpm, w.run_cnt, w.runs_pitch, w.tempo);
}

void launch_beat(const Batch& b, const Workspace& w, const DeviceTables& t, hipStream_t st) {
    launch_beat_acf(b, w, t, st);
    launch_beat_track(b, w, t, st);
}

}  // namespace bg
