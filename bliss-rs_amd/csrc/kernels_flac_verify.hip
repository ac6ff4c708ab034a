// kernels_flac_verify.hip -- the opt-in integrity checks of the FLAC path: every frame's CRC-16, every song's MD5.
//
// flac_crc_kernel: one wavefront per frame.  The lanes take the frame's aligned 8-byte words round-robin (a wavefront's load
// is 512 consecutive bytes), each folds its words with one Horner step by x^(8 * 512) per round, shifts its partial value by
// its true trailing byte count, and the 64 values are xor-reduced across the wavefront (flac_verify.hpp: crc16_lane, the text
// the CPU tests run lane by lane).  The frame's range is [offset, end[i]): the decoder's own stop position, so bytes behind the
// last frame's audio (an ID3v1 tag, padding) are not taken for it.  The range is checked against the table row and the file
// before the first load; a range that fails is a CRC failure, never a load.
//
// flac_md5_kernel: one lane per song -- MD5 is serial per stream -- over the song's own PCM region, songs handed to lanes
// longest first so that a wavefront's lanes finish together.  A dependent chain of several hundred instructions per 64 bytes:
// slow for long songs, and only run when asked for.
#include <hip/hip_runtime.h>

#include "flac_frame.hpp"
#include "flac_verify.hpp"
#include "internal.hpp"

namespace bg {

namespace {

constexpr int CRC_WAVES = 4;  // frames (wavefronts) per workgroup

__global__ __launch_bounds__(CRC_WAVES * 64) void flac_crc_kernel(const uint8_t* __restrict__ bytes, const FlacSong* __restrict__ songs,
                                                                 const FlacFrame* __restrict__ frames, uint32_t n_frames,
                                                                 const int32_t* __restrict__ status, const uint64_t* __restrict__ end,
                                                                 const uint32_t* __restrict__ song_first, uint32_t* song_crc_bad,
                                                                 uint32_t* song_first_bad, int32_t* __restrict__ frame_ok) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * CRC_WAVES + (threadIdx.x >> 6);  // the same for the 64 lanes of a wavefront
    if (i >= n_frames) return;
    if (status[i] != flac::FRAME_OK) {
        if (frame_ok && lane == 0) frame_ok[i] = -1;
        return;
    }
    const FlacFrame f = frames[i];
    const uint32_t si = f.song & ~FLAC_LAST_FRAME;
    const FlacSong s = songs[si];
    const uint64_t stop = end[i];
    // header to CRC-16 inside the row, the row inside the file: all that follows loads inside [file, file + nbytes + 16)
    bool ok = f.offset <= s.nbytes && f.nbytes <= s.nbytes - f.offset && stop > f.offset && stop - f.offset + 2 <= f.nbytes;
    if (ok) {
        const uint8_t* file = bytes + s.byte_off;
        uint32_t c = flac::crc16_lane(file, f.offset, stop, lane);
        for (int m = 32; m >= 1; m >>= 1) c ^= (uint32_t)__shfl_xor((int)c, m, 64);
        ok = c == (((uint32_t)file[stop] << 8) | file[stop + 1]);
    }
    if (lane != 0) return;
    if (frame_ok) frame_ok[i] = ok ? 1 : 0;
    if (!ok && song_crc_bad) {
        song_crc_bad[si] = 1;
        atomicMin(&song_first_bad[si], i - song_first[si]);
    }
}

struct Md5Result { uint32_t w[4]; };

__global__ __launch_bounds__(64) void flac_md5_kernel(const uint8_t* __restrict__ pcm, const FlacMd5Job* __restrict__ jobs, uint32_t n_jobs,
                                                     Md5Result* __restrict__ digests, FlacMd5Job one) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n_jobs) return;
    const FlacMd5Job job = jobs ? jobs[t] : one;  // (jobs == NULL: the one job that came with the launch)
    Md5Result r;
    flac::md5_pcm(pcm + job.pcm_off, job.n_elems, job.bps, r.w);
    digests[job.slot] = r;
}

}  // namespace

void launch_flac_crc(const uint8_t* bytes, const FlacSong* songs, const FlacFrame* frames, uint32_t n_frames, const int32_t* status,
                     const uint64_t* end, const uint32_t* song_first, uint32_t* song_crc_bad, uint32_t* song_first_bad, int32_t* frame_ok,
                     hipStream_t st) {
    if (!n_frames) return;
    flac_crc_kernel<<<(n_frames + CRC_WAVES - 1) / CRC_WAVES, CRC_WAVES * 64, 0, st>>>(bytes, songs, frames, n_frames, status, end, song_first,
                                                                                       song_crc_bad, song_first_bad, frame_ok);
}

void launch_flac_md5(const uint8_t* pcm, const FlacMd5Job* jobs, uint32_t n_jobs, void* digests, hipStream_t st) {
    if (!n_jobs) return;
    flac_md5_kernel<<<(n_jobs + 63) / 64, 64, 0, st>>>(pcm, jobs, n_jobs, (Md5Result*)digests, FlacMd5Job{});
}

void launch_flac_md5_one(const uint8_t* pcm, const FlacMd5Job& job, void* digests, hipStream_t st) {
    flac_md5_kernel<<<1, 64, 0, st>>>(pcm, nullptr, 1, (Md5Result*)digests, job);
}

}  // namespace bg
