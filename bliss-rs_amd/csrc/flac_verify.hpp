// flac_verify.hpp -- the two integrity checks of a FLAC stream, written once for the host and the device.
//
// Plain C++17, no HIP types, no inline assembly, no lookup array: g++ and clang++ compile it for the CPU tests
// (tests/cpp/test_flac_verify.cpp), hipcc compiles the same text into flac_crc_kernel and flac_md5_kernel
// (kernels_flac_verify.hip).
//
// CRC-16 as FLAC defines it: polynomial x^16 + x^15 + x^2 + 1 (0x8005), initial value 0, most significant bit first, nothing
// reflected, over a frame from its first header byte up to (not including) the two CRC bytes.  With the initial value 0 the
// register IS the remainder M(x) * x^16 mod P, and the code is linear:
//     * leading zero bytes do not change it;
//     * crc(A || B) = crc(A) * x^(8 |B|) mod P  xor  crc(B).
// That is what lets 64 lanes share a frame: lane l takes the aligned 8-byte words l, l + 64, ... of the frame (the bytes in
// front of the frame's first byte masked to zero, the last word cut to the bytes the frame owns), folds them with one Horner
// step by x^(8 * 512) per round, and shifts its partial value by the bytes that follow its last word; the frame's CRC is the
// xor of the 64 values.
//
// Bounds: every load is an aligned 8-byte word that holds at least one byte of [begin, end), end <= nbytes: none lies
// outside [file, file + nbytes + 16) -- flac_frame.hpp's contract (16 readable bytes behind the file).
//
// MD5 (RFC 1321) over the FLAC message: the samples interleaved, each a little-endian signed value in ceil(bps / 8) bytes.
// The PCM holds sample << (16 - bps) as int16 (bps <= 16) or sample << (32 - bps) as int32: the packer shifts back
// arithmetically and emits 1, 2 or 3 bytes per sample.  Every load is guarded by the element count of the song's own region.
// The block function is fully unrolled; schedule and constants are fixed at compile time, the 16 message words stay in registers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if !defined(FLAC_HD)
#if defined(__HIPCC__)
#define FLAC_HD __host__ __device__
#else
#define FLAC_HD
#endif
#endif
#if !defined(FLAC_UNROLL)
#if defined(__clang__)
#define FLAC_UNROLL _Pragma("unroll")
#else
#define FLAC_UNROLL
#endif
#endif

namespace flac {

// ---- CRC-16 ----
constexpr uint32_t CRC16_POLY = 0x8005;
constexpr uint32_t CRC_LANES = 64;               // lanes that share a frame
constexpr uint32_t CRC_ROUND_BYTES = 8 * CRC_LANES;  // bytes one round of the 64 lanes covers

// One byte into the register: c' = (c * x^8 + b * x^16) mod P.  The eight bits q that leave the register come back as
// q * x^16 mod P.  x^(16 + k) mod P = x^15 + (x^2 + 1)(1 + x + .. + x^k) for k = 0..7, so with s_j = parity of q's bits j..7:
// q * x^16 mod P = s_0 * x^15 + (x^2 + 1) * (s_7 .. s_0) -- three shifts and xors for the suffix parities, no table.
FLAC_HD constexpr uint32_t crc16_byte(uint32_t c, uint32_t b) {
    uint32_t q = ((c >> 8) ^ b) & 0xFF;
    q ^= q >> 1;
    q ^= q >> 2;
    q ^= q >> 4;
    return ((c << 8) & 0xFF00) ^ ((q & 1) << 15) ^ q ^ (q << 2);
}

// the definition, bit by bit (what the tests hold crc16_byte to)
FLAC_HD constexpr uint32_t crc16_bitwise(uint32_t c, uint32_t b) {
    c ^= b << 8;
    for (int i = 0; i < 8; i++) c = (c & 0x8000) ? ((c << 1) ^ CRC16_POLY) & 0xFFFF : (c << 1) & 0xFFFF;
    return c;
}

FLAC_HD inline uint32_t crc16_serial(const uint8_t* p, size_t n, uint32_t c = 0) {
    for (size_t i = 0; i < n; i++) c = crc16_byte(c, p[i]);
    return c;
}

// the CRC of the 8 bytes of a big-endian word, from 0 (leading zero bytes are free)
FLAC_HD constexpr uint32_t crc16_word(uint64_t be) {
    uint32_t c = 0;
    for (int i = 7; i >= 0; i--) c = crc16_byte(c, (uint32_t)(be >> (8 * i)) & 0xFF);
    return c;
}

// carry-less a * b mod P, both below x^16
FLAC_HD constexpr uint32_t crc16_mul(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 15; i >= 0; i--) {
        r = ((r << 1) & 0xFFFF) ^ ((r & 0x8000) ? CRC16_POLY : 0u);
        r ^= ((b >> i) & 1) ? a : 0u;
    }
    return r;
}

// x^(8 n) mod P by repeated squaring
FLAC_HD constexpr uint32_t crc16_xpow8(uint64_t n) {
    uint32_t r = 1, s = 0x100;
    while (n) {
        if (n & 1) r = crc16_mul(r, s);
        s = crc16_mul(s, s);
        n >>= 1;
    }
    return r;
}

// crc(A || B) from crc(A), crc(B) and |B|
FLAC_HD constexpr uint32_t crc16_combine(uint32_t crc_a, uint32_t crc_b, uint64_t nbytes_b) {
    return crc16_mul(crc_a, crc16_xpow8(nbytes_b)) ^ crc_b;
}

constexpr uint32_t CRC16_X_ROUND = crc16_xpow8(CRC_ROUND_BYTES);  // the Horner step of one round

FLAC_HD inline uint64_t crc_load_be64(const uint8_t* base, uint64_t word) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bswap64(reinterpret_cast<const uint64_t*>(base)[word]);  // aligned 8-byte load
#else
    uint64_t v;
    memcpy(&v, base + word * 8, 8);
    return __builtin_bswap64(v);
#endif
}

// Lane `lane` of CRC_LANES over the bytes [begin, end) of `file`, begin < end: its share of the frame's CRC, already
// shifted to the frame's end.  The xor over the lanes is the CRC.  `file` is 8-byte aligned on the device.
FLAC_HD inline uint32_t crc16_lane(const uint8_t* file, uint64_t begin, uint64_t end, uint32_t lane) {
    const uint64_t w0 = begin >> 3, wl = (end - 1) >> 3, nwords = wl - w0 + 1;
    const uint64_t nfull = nwords - 1;                // the words in front of the last one: whole 8 bytes each
    const uint64_t head_mask = ~0ull >> (8 * (begin & 7));  // drops the bytes of word 0 in front of the frame
    const uint32_t tail = (uint32_t)(end - wl * 8);   // bytes of the last word the frame owns, 1..8
    uint32_t c = 0;
    if (lane < nfull) {
        uint64_t j = lane;
        for (;; j += CRC_LANES) {
            uint64_t v = crc_load_be64(file, w0 + j);
            if (j == 0) v &= head_mask;
            c = crc16_mul(c, CRC16_X_ROUND) ^ crc16_word(v);
            if (j + CRC_LANES >= nfull) break;
        }
        const uint64_t behind = end - (w0 + j + 1) * 8;  // the lane's true trailing byte count, 1..512
        c = crc16_mul(c, crc16_xpow8(behind));
    }
    if (lane == nfull % CRC_LANES) {  // the last word goes to the lane whose turn it is, cut to the frame's own bytes
        uint64_t v = crc_load_be64(file, wl);
        if (nfull == 0) v &= head_mask;
        c ^= crc16_word(v >> (8 * (8 - tail)));
    }
    return c;
}

// the 64 lanes one after the other (host form; the device reduces them across the wavefront)
inline uint32_t crc16_lanes(const uint8_t* file, uint64_t begin, uint64_t end) {
    uint32_t c = 0;
    if (begin < end)
        for (uint32_t l = 0; l < CRC_LANES; l++) c ^= crc16_lane(file, begin, end, l);
    return c;
}

// ---- MD5 ----
struct Md5State {
    uint32_t a = 0x67452301, b = 0xefcdab89, c = 0x98badcfe, d = 0x10325476;
};

FLAC_HD inline uint32_t md5_rotl(uint32_t v, int s) { return (v << s) | (v >> (32 - s)); }

#define FLAC_MD5_F(x, y, z) ((z) ^ ((x) & ((y) ^ (z))))
#define FLAC_MD5_G(x, y, z) ((y) ^ ((z) & ((x) ^ (y))))
#define FLAC_MD5_H(x, y, z) ((x) ^ (y) ^ (z))
#define FLAC_MD5_I(x, y, z) ((y) ^ ((x) | ~(z)))
#define FLAC_MD5_STEP(f, a, b, c, d, k, s, t) a = md5_rotl(a + f(b, c, d) + w[k] + t, s) + b
#define FLAC_MD5_R4(f, k0, k1, k2, k3, s0, s1, s2, s3, t0, t1, t2, t3) \
    FLAC_MD5_STEP(f, a, b, c, d, k0, s0, t0);                          \
    FLAC_MD5_STEP(f, d, a, b, c, k1, s1, t1);                          \
    FLAC_MD5_STEP(f, c, d, a, b, k2, s2, t2);                          \
    FLAC_MD5_STEP(f, b, c, d, a, k3, s3, t3)

// one 64-byte block, w = its 16 little-endian words (constant indices only: they stay in registers)
FLAC_HD inline void md5_block(Md5State& st, const uint32_t* w) {
    uint32_t a = st.a, b = st.b, c = st.c, d = st.d;
    FLAC_MD5_R4(FLAC_MD5_F, 0, 1, 2, 3, 7, 12, 17, 22, 0xd76aa478u, 0xe8c7b756u, 0x242070dbu, 0xc1bdceeeu);
    FLAC_MD5_R4(FLAC_MD5_F, 4, 5, 6, 7, 7, 12, 17, 22, 0xf57c0fafu, 0x4787c62au, 0xa8304613u, 0xfd469501u);
    FLAC_MD5_R4(FLAC_MD5_F, 8, 9, 10, 11, 7, 12, 17, 22, 0x698098d8u, 0x8b44f7afu, 0xffff5bb1u, 0x895cd7beu);
    FLAC_MD5_R4(FLAC_MD5_F, 12, 13, 14, 15, 7, 12, 17, 22, 0x6b901122u, 0xfd987193u, 0xa679438eu, 0x49b40821u);
    FLAC_MD5_R4(FLAC_MD5_G, 1, 6, 11, 0, 5, 9, 14, 20, 0xf61e2562u, 0xc040b340u, 0x265e5a51u, 0xe9b6c7aau);
    FLAC_MD5_R4(FLAC_MD5_G, 5, 10, 15, 4, 5, 9, 14, 20, 0xd62f105du, 0x02441453u, 0xd8a1e681u, 0xe7d3fbc8u);
    FLAC_MD5_R4(FLAC_MD5_G, 9, 14, 3, 8, 5, 9, 14, 20, 0x21e1cde6u, 0xc33707d6u, 0xf4d50d87u, 0x455a14edu);
    FLAC_MD5_R4(FLAC_MD5_G, 13, 2, 7, 12, 5, 9, 14, 20, 0xa9e3e905u, 0xfcefa3f8u, 0x676f02d9u, 0x8d2a4c8au);
    FLAC_MD5_R4(FLAC_MD5_H, 5, 8, 11, 14, 4, 11, 16, 23, 0xfffa3942u, 0x8771f681u, 0x6d9d6122u, 0xfde5380cu);
    FLAC_MD5_R4(FLAC_MD5_H, 1, 4, 7, 10, 4, 11, 16, 23, 0xa4beea44u, 0x4bdecfa9u, 0xf6bb4b60u, 0xbebfbc70u);
    FLAC_MD5_R4(FLAC_MD5_H, 13, 0, 3, 6, 4, 11, 16, 23, 0x289b7ec6u, 0xeaa127fau, 0xd4ef3085u, 0x04881d05u);
    FLAC_MD5_R4(FLAC_MD5_H, 9, 12, 15, 2, 4, 11, 16, 23, 0xd9d4d039u, 0xe6db99e5u, 0x1fa27cf8u, 0xc4ac5665u);
    FLAC_MD5_R4(FLAC_MD5_I, 0, 7, 14, 5, 6, 10, 15, 21, 0xf4292244u, 0x432aff97u, 0xab9423a7u, 0xfc93a039u);
    FLAC_MD5_R4(FLAC_MD5_I, 12, 3, 10, 1, 6, 10, 15, 21, 0x655b59c3u, 0x8f0ccc92u, 0xffeff47du, 0x85845dd1u);
    FLAC_MD5_R4(FLAC_MD5_I, 8, 15, 6, 13, 6, 10, 15, 21, 0x6fa87e4fu, 0xfe2ce6e0u, 0xa3014314u, 0x4e0811a1u);
    FLAC_MD5_R4(FLAC_MD5_I, 4, 11, 2, 9, 6, 10, 15, 21, 0xf7537e82u, 0xbd3af235u, 0x2ad7d2bbu, 0xeb86d391u);
    st.a += a;
    st.b += b;
    st.c += c;
    st.d += d;
}

#undef FLAC_MD5_R4
#undef FLAC_MD5_STEP
#undef FLAC_MD5_F
#undef FLAC_MD5_G
#undef FLAC_MD5_H
#undef FLAC_MD5_I

// RFC 1321's padding on the word at message offset m (a multiple of 4) of a message of len bytes: v holds the message's
// bytes (anything behind the message's end is dropped here)
FLAC_HD inline uint32_t md5_pad_word(uint32_t v, uint64_t len, uint64_t m) {
    if (m + 4 <= len) return v;
    if (m > len) return 0;
    const uint32_t r = (uint32_t)(len - m);  // 0..3 message bytes in this word, then the 0x80
    return (v & ((1u << (8 * r)) - 1)) | (0x80u << (8 * r));
}

// The digest of a message of len bytes whose 4-byte words come from fetch(block, j) (word j = 0..15 of 64-byte block
// `block`; bytes behind the message's end may be anything).  digest: a, b, c, d -- 16 bytes in little-endian order.
template <class Fetch>
FLAC_HD inline void md5_run(uint64_t len, Fetch fetch, uint32_t* digest) {
    Md5State st;
    const uint64_t nblk = (len + 8) / 64 + 1;
    for (uint64_t blk = 0; blk < nblk; blk++) {
        uint32_t w[16];
        if (blk * 64 + 64 <= len) {
            FLAC_UNROLL
            for (int j = 0; j < 16; j++) w[j] = fetch(blk, (uint32_t)j);
        } else {
            FLAC_UNROLL
            for (int j = 0; j < 16; j++) w[j] = md5_pad_word(fetch(blk, (uint32_t)j), len, blk * 64 + 4 * (uint64_t)j);
            if (blk == nblk - 1) {
                w[14] = (uint32_t)(len << 3);
                w[15] = (uint32_t)(len >> 29);
            }
        }
        md5_block(st, w);
    }
    digest[0] = st.a;
    digest[1] = st.b;
    digest[2] = st.c;
    digest[3] = st.d;
}

// a message in memory (host tests: the RFC's test suite)
struct Md5Bytes {
    const uint8_t* p;
    uint64_t n;
    FLAC_HD uint32_t operator()(uint64_t blk, uint32_t j) const {
        const uint64_t m = blk * 64 + 4 * (uint64_t)j;
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4; k++)
            if (m + k < n) v |= (uint32_t)p[m + k] << (8 * k);
        return v;
    }
};

// The FLAC message of a song's PCM region: n_elems = total x channels elements, int16 (bps <= 16) or int32.  An element at
// or behind n_elems reads as 0 and is never loaded.  pcm is 4-byte aligned.
struct Md5Pcm {
    const void* pcm;
    uint64_t n_elems;
    uint32_t bps;

    FLAC_HD static uint32_t width_of(uint32_t bps) { return (bps + 7) / 8; }
    FLAC_HD uint64_t message_bytes() const { return n_elems * width_of(bps); }

    // elements e, e + 1 of an int16 region as one word (e even)
    FLAC_HD uint32_t pair16(uint64_t e) const {
        if (e + 1 < n_elems) {
#if defined(__HIP_DEVICE_COMPILE__)
            return reinterpret_cast<const uint32_t*>(pcm)[e >> 1];  // aligned 4-byte load
#else
            uint32_t v;
            memcpy(&v, (const uint8_t*)pcm + 2 * e, 4);
            return v;
#endif
        }
        if (e < n_elems) {
            uint16_t v;
            memcpy(&v, (const uint8_t*)pcm + 2 * e, 2);
            return v;
        }
        return 0;
    }
    // element e of an int32 region, shifted back, its low 24 bits
    FLAC_HD uint32_t s24(uint64_t e) const {
        if (e >= n_elems) return 0;
        int32_t v;
        memcpy(&v, (const uint8_t*)pcm + 4 * e, 4);
        return (uint32_t)(v >> (32 - bps)) & 0xFFFFFFu;
    }

    FLAC_HD uint32_t operator()(uint64_t blk, uint32_t j) const {
        const uint32_t width = width_of(bps);
        if (width == 2) {  // two samples per word
            const uint32_t v = pair16(blk * 32 + 2 * (uint64_t)j), sh = 16 - bps;
            const uint32_t lo = (uint32_t)((int32_t)(v << 16) >> (16 + sh)) & 0xFFFFu;
            const uint32_t hi = (uint32_t)((int32_t)v >> (16 + sh)) & 0xFFFFu;
            return lo | (hi << 16);
        }
        if (width == 1) {  // four samples per word
            const uint64_t e = blk * 64 + 4 * (uint64_t)j;
            const uint32_t v0 = pair16(e), v1 = pair16(e + 2), sh = 16 - bps;
            const uint32_t b0 = (uint32_t)((int32_t)(v0 << 16) >> (16 + sh)) & 0xFFu, b1 = (uint32_t)((int32_t)v0 >> (16 + sh)) & 0xFFu;
            const uint32_t b2 = (uint32_t)((int32_t)(v1 << 16) >> (16 + sh)) & 0xFFu, b3 = (uint32_t)((int32_t)v1 >> (16 + sh)) & 0xFFu;
            return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
        }
        // three bytes per sample: the word at message offset m = 64 blk + 4 j starts at byte k = m % 3 of sample m / 3 and
        // ends in the next sample
        const uint64_t e0 = (blk * 64) / 3;
        const uint32_t t = (uint32_t)((blk * 64) % 3) + 4 * j;
        const uint64_t e = e0 + t / 3;
        const uint32_t k = t % 3;
        return (s24(e) >> (8 * k)) | (s24(e + 1) << (24 - 8 * k));
    }
};

// digest (16 bytes) of the FLAC message of a PCM region
FLAC_HD inline void md5_pcm(const void* pcm, uint64_t n_elems, uint32_t bps, uint32_t* digest) {
    const Md5Pcm f{pcm, n_elems, bps};
    md5_run(f.message_bytes(), f, digest);
}

}  // namespace flac
