// kernels_flac.hip -- FLAC frames -> interleaved PCM on the device, one lane per frame.
//
// Rice decoding is serial within a frame, and a subframe's start is only known once the one before it has been parsed: the
// frame is the unit of parallelism.  64 consecutive rows of the frame table make a wavefront; rows continue across song
// boundaries, so the tail of one song and the head of the next share a wavefront.  A batch of 256 three-minute songs has
// about half a million frames.
//
// The decoding itself is flac_frame.hpp, the same text the CPU tests run under a sanitizer: its loads stay inside
// [file, file + nbytes + 16), its stores inside the frame's own region of the song's PCM.  Here only the predictor window of
// orders 13..32 is added: 64 words per lane in LDS, laid out [tap][lane] (lane l reads bank l % 64 whatever the tap: no two
// lanes of a wavefront meet in a bank).  Orders up to 12 keep their history in registers (flac::RegHist).
//
// Store form: one sample per lane per store, a whole frame apart from its neighbour lane's (the plain form; the staged form
// was measured slower and is not kept: DESIGN.md section 3.18).
#include <hip/hip_runtime.h>

#include "flac_frame.hpp"
#include "internal.hpp"

namespace bg {

namespace {

struct LdsWin {
    int32_t* p;  // this lane's column
    __device__ int32_t& at(uint32_t k) { return p[k * FLAC_LANES]; }
};

__global__ __launch_bounds__(FLAC_LANES) void flac_decode_kernel(const uint8_t* __restrict__ bytes, const FlacSong* __restrict__ songs,
                                                                const FlacFrame* __restrict__ frames, uint32_t n_frames,
                                                                uint8_t* pcm, int32_t* __restrict__ status,
                                                                uint64_t* __restrict__ end) {
    __shared__ int32_t window[64 * FLAC_LANES];
    const uint32_t i = blockIdx.x * FLAC_LANES + threadIdx.x;
    if (i >= n_frames) return;
    const FlacFrame f = frames[i];
    const FlacSong s = songs[f.song & ~FLAC_LAST_FRAME];
    LdsWin win{window + threadIdx.x};
    uint64_t stop = 0;
    const int st = flac::decode_frame(bytes + s.byte_off, s.nbytes, f.offset, f.nbytes, f.first_sample, f.blocksize, s.channels, s.bps,
                                      s.total, s.base, pcm + s.pcm_off, win, &stop);
    status[i] = st;
    end[i] = stop;
}

// frame i has to be sound and to stop exactly 2 bytes (its CRC-16) before the next frame of the table / the end of the data
__global__ void flac_check_kernel(const FlacFrame* __restrict__ frames, uint32_t n_frames, const int32_t* __restrict__ status,
                                  const uint64_t* __restrict__ end, uint32_t* __restrict__ song_bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_frames) return;
    const FlacFrame f = frames[i];
    const bool last = (f.song & FLAC_LAST_FRAME) != 0;
    const uint64_t stop = end[i] + 2, want = f.offset + f.nbytes;
    if (status[i] != flac::FRAME_OK || (last ? stop > want : stop != want)) song_bad[f.song & ~FLAC_LAST_FRAME] = 1;
}

}  // namespace

void launch_flac_decode(const uint8_t* bytes, const FlacSong* songs, const FlacFrame* frames, uint32_t n_frames, uint8_t* pcm,
                        int32_t* status, uint64_t* end, hipStream_t st) {
    if (!n_frames) return;
    const dim3 grid((n_frames + FLAC_LANES - 1) / FLAC_LANES);
    flac_decode_kernel<<<grid, FLAC_LANES, 0, st>>>(bytes, songs, frames, n_frames, pcm, status, end);
}

void launch_flac_check(const FlacFrame* frames, uint32_t n_frames, const int32_t* status, const uint64_t* end, uint32_t* song_bad,
                       hipStream_t st) {
    if (!n_frames) return;
    flac_check_kernel<<<(n_frames + 255) / 256, 256, 0, st>>>(frames, n_frames, status, end, song_bad);
}

}  // namespace bg
