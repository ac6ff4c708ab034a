// flac_frame.hpp -- one FLAC frame -> interleaved PCM, written once for the host and the device.
//
// Plain C++17, no HIP types, no inline assembly: g++ and clang++ compile it for the CPU tests (tests/cpp/test_flac.cpp),
// hipcc compiles the same text into flac_decode_kernel (kernels_flac.hip), one lane per frame.
//
// Bounds are structural:
//   * loads   every load is an 8-byte word of the bit reader.  The reader never moves past the frame's last bit, the frame lies
//             inside the file (checked first), and the words it holds are the one under the cursor and the next one: no load lies
//             outside [file, file + nbytes + 16).  The caller pads 16 bytes behind the file; `file` is 8-byte aligned on the device.
//   * stores  every store goes through Emit::put, which drops sample i >= nvalid = min(blocksize, total - first_sample): nothing
//             is written outside the frame's own blocksize x channels region, clipped to the stream's total.
//   * loops   every loop runs to the block size, a partition count (each turn consumes bits) or the frame's end; a unary run
//             stops at the frame's last bit.  Once the reader has been refused a bit it stays refused and the loops wind down.
// A violation is a frame status, never a fault.  Not checked here: CRC-8, CRC-16, the stream MD5.  flac_index.hpp checks the
// CRCs on the host when asked to; on the device the CRC-16 and the MD5 are flac_verify.hpp's (flac_crc_kernel and
// flac_md5_kernel, kernels_flac_verify.hip), run when a caller asks for them.
//
// Prediction sums are 64-bit for every subframe (one v_mad_i64_i32 per tap on gfx950): exact for every valid stream, and
// equal to libFLAC's 32-bit path wherever the format allows that path.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define FLAC_HD __host__ __device__
#else
#define FLAC_HD
#endif
#if defined(__clang__)
#define FLAC_UNROLL _Pragma("unroll")
#else
#define FLAC_UNROLL
#endif

namespace flac {

enum FrameStatus : int32_t {
    FRAME_OK = 0,
    FRAME_RESERVED_TYPE = 1,        // reserved subframe type, or its padding bit set
    FRAME_RESERVED_ASSIGNMENT = 2,  // channel assignment 11..15
    FRAME_HEADER_MISMATCH = 3,      // no sync, reserved bits, or block size / depth / channels / position that are not the table's
    FRAME_OVERRUN = 4,              // ran past the frame (or the frame does not lie inside the file)
    FRAME_NEGATIVE_SHIFT = 5,       // LPC quantisation shift < 0
    FRAME_UNSUPPORTED_DEPTH = 6,    // outside 4..24 bits per sample (32-bit streams need a 33-bit side channel)
    FRAME_BAD_SUBFRAME = 7,         // wasted bits >= depth, reserved residual method / precision, predictor order above the
                                    // block or the first partition, block size no multiple of the partition count
    FRAME_NOT_RUN = 8,              // (initial value of a status array)
};

constexpr uint32_t MAX_FRAME_BYTES = 1u << 24;  // 65 535 samples x 8 channels x 32 bits and every header fit many times over
constexpr uint32_t FILE_PAD = 16;               // bytes the caller keeps readable behind the file

FLAC_HD inline uint64_t load_be64(const uint8_t* base, size_t word) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bswap64(reinterpret_cast<const uint64_t*>(base)[word]);  // aligned 8-byte load
#else
    uint64_t v;
    memcpy(&v, base + word * 8, 8);
    return __builtin_bswap64(v);
#endif
}

// Big-endian bit reader over one frame.  `left` counts the bits the frame still has; a read that wants more is refused:
// it returns 0, moves nothing and sets `over`.
struct BitReader {
    const uint8_t* base;
    uint64_t cur, next;  // the word under the cursor and the one behind it
    size_t w;            // index of `cur`
    uint32_t bp;         // bits of `cur` already consumed, 0..63
    uint32_t left;
    bool over;

    FLAC_HD void init(const uint8_t* file, uint64_t byte_off, uint32_t nbytes) {
        base = file;
        w = (size_t)(byte_off >> 3);
        bp = (uint32_t)(byte_off & 7) * 8;
        left = nbytes * 8;
        over = false;
        cur = load_be64(base, w);
        next = load_be64(base, w + 1);
    }
    FLAC_HD uint64_t peek() const { return bp ? (cur << bp) | (next >> (64 - bp)) : cur; }
    FLAC_HD void skip(uint32_t n) {  // n <= 64 and n <= left
        left -= n;
        bp += n;
        if (bp >= 64) {
            bp -= 64;
            w++;
            cur = next;
            next = load_be64(base, w + 1);
        }
    }
    FLAC_HD bool refuse() {
        over = true;
        left = 0;
        return true;
    }
    FLAC_HD uint32_t read(uint32_t n) {  // n = 0..32
        if (n == 0) return 0;
        if (n > left) { refuse(); return 0; }
        const uint32_t v = (uint32_t)(peek() >> (64 - n));
        skip(n);
        return v;
    }
    FLAC_HD int32_t read_signed(uint32_t n) {
        if (n == 0) return 0;
        const uint32_t v = read(n);
        return (int32_t)(v << (32 - n)) >> (32 - n);
    }
    FLAC_HD uint32_t unary() {  // zero bits before the next one bit
        uint32_t q = 0;
        for (;;) {
            const uint64_t win = peek();
            if (win == 0) {
                if (left < 64) { refuse(); return q; }
                skip(64);
                q += 64;
                continue;
            }
            const uint32_t z = (uint32_t)__builtin_clzll(win);
            if (z + 1 > left) { refuse(); return q; }
            skip(z + 1);
            return q + z;
        }
    }
    FLAC_HD void align() {
        const uint32_t n = (8 - (bp & 7)) & 7;
        if (n > left) { refuse(); return; }
        if (n) skip(n);
    }
    FLAC_HD uint64_t byte_pos() const { return (uint64_t)w * 8 + (bp >> 3); }
};

// Where a frame's samples go.  Up to 16 bits per sample: int16, sample << (16 - bps); above: int32, sample << (32 - bps) --
// what the reference's FFmpeg decoder hands on.  Channel 0 of a decorrelated pair is written to its slot as decoded (its low
// bits: a 17-bit side channel of a 16-bit stream keeps its low 16, which is all the sum below needs); the lane reads it back
// when it decodes channel 1 and rewrites both.
enum Role : int { ROLE_PLAIN = 0, ROLE_RAW = 1, ROLE_LEFT_SIDE = 2, ROLE_SIDE_RIGHT = 3, ROLE_MID_SIDE = 4 };

// Store form: plain -- one element per store.  On the device that is 64 write transactions per store instruction, a frame
// apart; staging 16-element runs per lane through LDS into 16-byte stores was built and measured and is slower (the lane's
// serial Rice / prediction chain is what the kernel waits for, not its stores): DESIGN.md section 3.18 has both times.
struct Emit {
    void* pcm;
    uint64_t first;     // first inter-channel sample of the frame
    uint32_t channels;
    uint32_t nvalid;    // samples of the frame below the stream's total
    uint32_t shift;     // 16 - bps or 32 - bps
    bool wide;          // int32 output

    FLAC_HD int32_t load(uint64_t idx) const {
        return wide ? static_cast<const int32_t*>(pcm)[idx] : (int32_t) static_cast<const int16_t*>(pcm)[idx];
    }
    FLAC_HD void store(uint64_t idx, uint32_t v) const {
        if (wide) static_cast<int32_t*>(pcm)[idx] = (int32_t)v;
        else static_cast<int16_t*>(pcm)[idx] = (int16_t)(uint16_t)v;
    }
    FLAC_HD void put(uint32_t i, uint32_t c, int role, int32_t v) const {
        if (i >= nvalid) return;
        const uint64_t idx = (first + i) * channels + c;
        if (role == ROLE_PLAIN) { store(idx, (uint32_t)v << shift); return; }
        if (role == ROLE_RAW) { store(idx, (uint32_t)v); return; }
        const uint32_t a = (uint32_t)load(idx - 1), b = (uint32_t)v;
        uint32_t l, r;
        if (role == ROLE_LEFT_SIDE) { l = a; r = a - b; }
        else if (role == ROLE_SIDE_RIGHT) { l = a + b; r = b; }
        else {
            const uint32_t m = (a << 1) | (b & 1);
            l = (uint32_t)((int32_t)(m + b) >> 1);
            r = (uint32_t)((int32_t)(m - b) >> 1);
        }
        store(idx - 1, l << shift);
        store(idx, r << shift);
    }
};

// Predictor state of orders up to N in registers: every index below is a compile-time constant once the loops are unrolled,
// so neither array is ever addressed at run time.  Taps above the subframe's order hold coefficient 0.
template <int N>
struct RegHist {
    int32_t h[N], c[N];
    FLAC_HD void clear() {
FLAC_UNROLL
        for (int j = 0; j < N; j++) { h[j] = 0; c[j] = 0; }
    }
    FLAC_HD void push(int32_t s) {
FLAC_UNROLL
        for (int j = N - 1; j > 0; j--) h[j] = h[j - 1];
        h[0] = s;
    }
    FLAC_HD void read_coefs(BitReader& br, uint32_t order, uint32_t prec) {
FLAC_UNROLL
        for (int j = 0; j < N; j++)
            if ((uint32_t)j < order) c[j] = br.read_signed(prec);
    }
    FLAC_HD void fixed_coefs(uint32_t order) {  // N >= 4
        c[0] = order == 1 ? 1 : order == 2 ? 2 : order == 3 ? 3 : order == 4 ? 4 : 0;
        c[1] = order == 2 ? -1 : order == 3 ? -3 : order == 4 ? -6 : 0;
        c[2] = order == 3 ? 1 : order == 4 ? 4 : 0;
        c[3] = order == 4 ? -1 : 0;
    }
    FLAC_HD int64_t sum(uint32_t) const {
        int64_t s = 0;
FLAC_UNROLL
        for (int j = 0; j < N; j++) s += (int64_t)c[j] * h[j];
        return s;
    }
};

// Orders 13..32: a 32-sample ring and 32 coefficients in a window the caller provides (Win::at(k), k = 0..63: the device
// keeps it in LDS laid out [tap][lane], the host in a plain array).
template <class Win>
struct WinHist {
    Win& win;
    uint32_t pos;
    FLAC_HD explicit WinHist(Win& w) : win(w), pos(0) {}
    FLAC_HD void clear() { pos = 0; }
    FLAC_HD void push(int32_t s) {
        win.at(pos & 31) = s;
        pos++;
    }
    FLAC_HD void read_coefs(BitReader& br, uint32_t order, uint32_t prec) {
        for (uint32_t j = 0; j < order && j < 32; j++) win.at(32 + j) = br.read_signed(prec);
    }
    FLAC_HD void fixed_coefs(uint32_t) {}
    FLAC_HD int64_t sum(uint32_t order) const {
        int64_t s = 0;
        for (uint32_t j = 0; j < order && j < 32; j++) s += (int64_t)win.at(32 + j) * win.at((pos - 1 - j) & 31);
        return s;
    }
};

struct HostWin {  // the window of the CPU build
    int32_t v[64];
    int32_t& at(uint32_t k) { return v[k]; }
};

// FIXED and LPC subframes behind the subframe header: warm-up samples, coefficients, residual, prediction.
template <class H>
FLAC_HD int predicted_subframe(BitReader& br, H& hist, bool lpc, uint32_t order, uint32_t bs, uint32_t bps, uint32_t wasted,
                               const Emit& em, uint32_t ch, int role) {
    hist.clear();
    for (uint32_t i = 0; i < order; i++) {
        const int32_t s = br.read_signed(bps);
        em.put(i, ch, role, (int32_t)((uint32_t)s << wasted));
        hist.push(s);
    }
    uint32_t shift = 0;
    if (lpc) {
        const uint32_t prec = br.read(4) + 1;
        if (prec == 16) return FRAME_BAD_SUBFRAME;
        const int32_t sh = br.read_signed(5);
        if (sh < 0) return FRAME_NEGATIVE_SHIFT;
        shift = (uint32_t)sh;
        hist.read_coefs(br, order, prec);
    } else {
        hist.fixed_coefs(order);
    }
    const uint32_t method = br.read(2);
    if (method > 1) return FRAME_BAD_SUBFRAME;
    const uint32_t pbits = method ? 5 : 4, esc = method ? 31 : 15;
    const uint32_t porder = br.read(4);
    const uint32_t psize = bs >> porder;
    if ((psize << porder) != bs || psize < order) return FRAME_BAD_SUBFRAME;
    uint32_t i = order;
    for (uint32_t part = 0; part < (1u << porder) && !br.over; part++) {
        const uint32_t cnt = psize - (part == 0 ? order : 0);
        const uint32_t k = br.read(pbits);
        const bool raw = k == esc;
        const uint32_t nb = raw ? br.read(5) : 0;
        for (uint32_t n = 0; n < cnt && !br.over; n++, i++) {
            int32_t r;
            if (raw) {
                r = br.read_signed(nb);
            } else {
                const uint32_t q = br.unary();
                const uint32_t v = (q << k) | br.read(k);
                r = (int32_t)((v >> 1) ^ (0u - (v & 1)));
            }
            const int64_t pred = hist.sum(order) >> shift;
            const int32_t s = (int32_t)(uint32_t)((uint64_t)pred + (uint64_t)(int64_t)r);
            em.put(i, ch, role, (int32_t)((uint32_t)s << wasted));
            hist.push(s);
        }
    }
    return FRAME_OK;
}

template <class Win>
FLAC_HD int decode_subframe(BitReader& br, uint32_t bs, uint32_t bps, const Emit& em, uint32_t ch, int role, Win& win) {
    if (br.read(1)) return FRAME_RESERVED_TYPE;
    const uint32_t type = br.read(6);
    uint32_t wasted = 0;
    if (br.read(1)) wasted = br.unary() + 1;
    if (br.over) return FRAME_OVERRUN;
    if (wasted >= bps) return FRAME_BAD_SUBFRAME;
    bps -= wasted;
    if (type == 0) {  // CONSTANT
        const int32_t v = (int32_t)((uint32_t)br.read_signed(bps) << wasted);
        for (uint32_t i = 0; i < bs; i++) em.put(i, ch, role, v);
        return FRAME_OK;
    }
    if (type == 1) {  // VERBATIM
        for (uint32_t i = 0; i < bs && !br.over; i++) em.put(i, ch, role, (int32_t)((uint32_t)br.read_signed(bps) << wasted));
        return FRAME_OK;
    }
    const bool lpc = type >= 32;
    if (!lpc && (type < 8 || type > 12)) return FRAME_RESERVED_TYPE;
    const uint32_t order = lpc ? (type & 31) + 1 : type - 8;
    if (order > bs) return FRAME_BAD_SUBFRAME;
    if (order <= 4) {
        RegHist<4> h;
        return predicted_subframe(br, h, lpc, order, bs, bps, wasted, em, ch, role);
    }
    if (order <= 8) {
        RegHist<8> h;
        return predicted_subframe(br, h, lpc, order, bs, bps, wasted, em, ch, role);
    }
    if (order <= 12) {
        RegHist<12> h;
        return predicted_subframe(br, h, lpc, order, bs, bps, wasted, em, ch, role);
    }
    WinHist<Win> h(win);
    return predicted_subframe(br, h, lpc, order, bs, bps, wasted, em, ch, role);
}

// One frame.  [off, off + len) is the frame's byte range in the file as the index found it (header to CRC-16); first_sample
// and blocksize are the index's too and the header, parsed again here, has to agree (a variable-block-size header codes
// number_base + first_sample).  `pcm` is the stream's whole output, total x channels samples.  *end_pos receives the byte position the decoder stopped at: off + len - 2 for a frame that
// is what the index took it for.
template <class Win>
FLAC_HD int decode_frame(const uint8_t* file, uint64_t file_nbytes, uint64_t off, uint64_t len, uint64_t first_sample,
                         uint32_t blocksize, uint32_t channels, uint32_t bps, uint64_t total, uint64_t number_base, void* pcm,
                         Win& win, uint64_t* end_pos) {
    *end_pos = off;
    if (bps < 4 || bps > 24) return FRAME_UNSUPPORTED_DEPTH;
    if (channels < 1 || channels > 8) return FRAME_HEADER_MISMATCH;
    if (off > file_nbytes || len > file_nbytes - off) return FRAME_OVERRUN;
    BitReader br;
    br.init(file, off, (uint32_t)(len < MAX_FRAME_BYTES ? len : MAX_FRAME_BYTES));
    int st = FRAME_OK;
    uint32_t assignment = 0;
    {
        const uint32_t sync = br.read(15);  // 14 sync bits and a reserved zero
        const uint32_t strategy = br.read(1);
        const uint32_t bsc = br.read(4), src = br.read(4);
        assignment = br.read(4);
        const uint32_t ssc = br.read(3), res = br.read(1);
        uint32_t b0 = br.read(8), follow = 0;
        while (follow < 8 && (b0 & (0x80u >> follow))) follow++;
        uint64_t number = follow ? (b0 & (0x7Fu >> follow)) : b0;
        bool bad = sync != 0x7FFC || res || follow == 1 || follow == 8 || bsc == 0 || src == 15 || ssc == 3;
        for (uint32_t j = 1; j < follow && j < 7; j++) {
            const uint32_t b = br.read(8);
            bad = bad || (b & 0xC0) != 0x80;
            number = (number << 6) | (b & 0x3F);
        }
        uint32_t bs = bsc == 1 ? 192 : bsc <= 5 ? 576u << (bsc - 2) : bsc == 6 ? br.read(8) + 1 : bsc == 7 ? br.read(16) + 1 : 256u << (bsc - 8);
        if (src == 12) br.read(8);
        else if (src == 13 || src == 14) br.read(16);
        br.read(8);  // CRC-8: the index has checked it
        const uint32_t depth = ssc == 0 ? bps : ssc == 1 ? 8 : ssc == 2 ? 12 : ssc == 4 ? 16 : ssc == 5 ? 20 : ssc == 6 ? 24 : 32;
        if (br.over) st = FRAME_OVERRUN;
        else if (bad) st = FRAME_HEADER_MISMATCH;
        else if (depth == 32) st = FRAME_UNSUPPORTED_DEPTH;
        else if (assignment > 10) st = FRAME_RESERVED_ASSIGNMENT;
        else if (bs != blocksize || depth != bps || (strategy && number != first_sample + number_base) ||
                 (assignment < 8 ? assignment + 1 : 2u) != channels)
            st = FRAME_HEADER_MISMATCH;
    }
    if (st == FRAME_OK) {
        Emit em;
        em.pcm = pcm;
        em.first = first_sample;
        em.channels = channels;
        em.nvalid = first_sample >= total ? 0 : (total - first_sample < blocksize ? (uint32_t)(total - first_sample) : blocksize);
        em.wide = bps > 16;
        em.shift = (em.wide ? 32 : 16) - bps;
        for (uint32_t c = 0; c < channels && st == FRAME_OK; c++) {
            int role = ROLE_PLAIN;
            uint32_t b = bps;
            if (assignment >= 8) {
                role = c == 0 ? ROLE_RAW : assignment == 8 ? ROLE_LEFT_SIDE : assignment == 9 ? ROLE_SIDE_RIGHT : ROLE_MID_SIDE;
                if ((assignment == 9) == (c == 0)) b++;  // the side channel carries one more bit
            }
            st = decode_subframe(br, blocksize, b, em, c, role, win);
            if (st == FRAME_OK && br.over) st = FRAME_OVERRUN;
        }
        if (st == FRAME_OK) {
            br.align();
            if (br.over) st = FRAME_OVERRUN;
        }
    }
    *end_pos = br.byte_pos();
    return st;
}

}  // namespace flac
