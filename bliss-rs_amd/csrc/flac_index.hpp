// flac_index.hpp -- the host half of the FLAC path, device-free: STREAMINFO and the frame table.
//
// flac::stream_info  optional ID3v2 tag, "fLaC", the metadata blocks -> rate, channels, depth, total, block / frame size
//                    limits, the MD5 and the offset of the first frame.
// flac::index_frames the frame table (byte offset, byte length, first sample, block size) in two modes:
//   fast      memchr for 0xFF from `min_framesize` behind the previous header on, the header parsed in full (reserved bits,
//             block-size code 0, sample-rate code 15, sample-size code 3, channel assignment above 10, rate / depth / channels
//             that disagree with STREAMINFO are rejected), CRC-8, and the coded frame or sample number has to be the one the
//             previous frame implies.  It never touches most bytes -- and a header-shaped run of bytes inside a frame fools it.
//             The decoder catches that: frame i has to stop exactly 2 bytes before frame i + 1 (flac_frame.hpp, *end_pos).
//   verified  the same plus CRC-16 over every candidate frame: candidates are walked until one closes, and the search starts
//             right behind the header whatever STREAMINFO's min_framesize says.  Exact for every frame but the last: that one
//             runs to the end of the data, and when its CRC-16 is not there (an ID3v1 tag, padding) the decoder's stop position
//             decides where it ended (`last_crc_ok` reports which it was).
// NOT checked on the hot path: CRC-16 (fast mode) and the stream MD5 (either mode).
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

namespace flac {

struct StreamInfo {
    uint32_t sample_rate = 0, channels = 0, bps = 0;
    uint64_t total = 0;  // 0: unknown
    uint32_t min_block = 0, max_block = 0, min_frame = 0, max_frame = 0;
    uint8_t md5[16] = {0};
    uint64_t first_frame = 0;     // byte offset of the first frame
};

struct FrameRow { uint64_t offset, nbytes, first_sample, blocksize; };

enum IndexError : int { INDEX_OK = 0, INDEX_NOT_FLAC = 1, INDEX_TRUNCATED = 2, INDEX_NO_FRAMES = 3 };

inline uint8_t crc8_byte(uint8_t crc, uint8_t b) {
    crc ^= b;
    for (int i = 0; i < 8; i++) crc = (uint8_t)((crc << 1) ^ ((crc & 0x80) ? 0x07 : 0));
    return crc;
}

struct Crc16Table {
    uint16_t t[256];
    Crc16Table() {
        for (int i = 0; i < 256; i++) {
            uint16_t c = (uint16_t)(i << 8);
            for (int k = 0; k < 8; k++) c = (uint16_t)((c << 1) ^ ((c & 0x8000) ? 0x8005 : 0));
            t[i] = c;
        }
    }
};
inline uint16_t crc16_update(uint16_t crc, const uint8_t* p, size_t n) {
    static const Crc16Table T;
    for (size_t i = 0; i < n; i++) crc = (uint16_t)((crc << 8) ^ T.t[(crc >> 8) ^ p[i]]);
    return crc;
}

inline int stream_info(const uint8_t* d, uint64_t n, StreamInfo* si) {
    uint64_t p = 0;
    if (n >= 10 && d[0] == 'I' && d[1] == 'D' && d[2] == '3') {  // ID3v2: four 7-bit size bytes, an optional 10-byte footer
        const uint64_t size = ((uint64_t)(d[6] & 0x7F) << 21) | ((uint64_t)(d[7] & 0x7F) << 14) | ((uint64_t)(d[8] & 0x7F) << 7) | (d[9] & 0x7F);
        p = 10 + size + ((d[5] & 0x10) ? 10 : 0);
    }
    if (p > n || n - p < 4 || memcmp(d + p, "fLaC", 4) != 0) return INDEX_NOT_FLAC;
    p += 4;
    bool have = false;
    for (;;) {
        if (n - p < 4) return INDEX_TRUNCATED;
        const uint8_t hdr = d[p];
        const uint64_t len = ((uint64_t)d[p + 1] << 16) | ((uint64_t)d[p + 2] << 8) | d[p + 3];
        p += 4;
        if (len > n - p) return INDEX_TRUNCATED;
        const uint8_t* b = d + p;
        if ((hdr & 0x7F) == 0) {
            if (len < 34) return INDEX_NOT_FLAC;
            si->min_block = (uint32_t)b[0] << 8 | b[1];
            si->max_block = (uint32_t)b[2] << 8 | b[3];
            si->min_frame = (uint32_t)b[4] << 16 | (uint32_t)b[5] << 8 | b[6];
            si->max_frame = (uint32_t)b[7] << 16 | (uint32_t)b[8] << 8 | b[9];
            uint64_t v = 0;
            for (int i = 10; i < 18; i++) v = (v << 8) | b[i];
            si->sample_rate = (uint32_t)(v >> 44);
            si->channels = (uint32_t)((v >> 41) & 7) + 1;
            si->bps = (uint32_t)((v >> 36) & 31) + 1;
            si->total = v & ((1ull << 36) - 1);
            memcpy(si->md5, b + 18, 16);
            have = true;
        }
        p += len;
        if (hdr & 0x80) break;
    }
    if (!have || si->sample_rate == 0) return INDEX_NOT_FLAC;
    si->first_frame = p;
    return INDEX_OK;
}

struct FrameHeader {
    uint32_t blocksize = 0, header_bytes = 0;
    bool variable = false;
    uint64_t number = 0;  // frame number (fixed block size) or first sample (variable)
};

// the header at d[p..] in full; false for anything that is not a frame header of THIS stream
inline bool parse_frame_header(const uint8_t* d, uint64_t n, uint64_t p, const StreamInfo& si, FrameHeader* h) {
    if (n - p < 6 || d[p] != 0xFF || (d[p + 1] & 0xFE) != 0xF8) return false;
    h->variable = d[p + 1] & 1;
    const uint32_t bsc = d[p + 2] >> 4, src = d[p + 2] & 15, ca = d[p + 3] >> 4, ssc = (d[p + 3] >> 1) & 7;
    if ((d[p + 3] & 1) || bsc == 0 || src == 15 || ssc == 3 || ca > 10) return false;
    uint64_t q = p + 4;
    const uint8_t b0 = d[q++];
    uint32_t follow = 0;
    while (follow < 8 && (b0 & (0x80u >> follow))) follow++;
    if (follow == 1 || follow == 8 || (follow == 7 && !h->variable)) return false;
    uint64_t number = follow ? (b0 & (0x7Fu >> follow)) : b0;
    for (uint32_t j = 1; j < follow; j++) {
        if (q >= n || (d[q] & 0xC0) != 0x80) return false;
        number = (number << 6) | (d[q++] & 0x3F);
    }
    h->number = number;
    uint32_t bs, rate = 0;
    if (bsc == 6) { if (n - q < 1) return false; bs = d[q] + 1u; q += 1; }
    else if (bsc == 7) { if (n - q < 2) return false; bs = (((uint32_t)d[q] << 8) | d[q + 1]) + 1u; q += 2; }
    else bs = bsc == 1 ? 192 : bsc <= 5 ? 576u << (bsc - 2) : 256u << (bsc - 8);
    static const uint32_t RATES[12] = {0, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000};
    if (src < 12) rate = RATES[src];
    else if (src == 12) { if (n - q < 1) return false; rate = d[q] * 1000u; q += 1; }
    else { if (n - q < 2) return false; rate = ((uint32_t)d[q] << 8) | d[q + 1]; if (src == 14) rate *= 10; q += 2; }
    if (q >= n) return false;
    static const uint32_t DEPTH[8] = {0, 8, 12, 0, 16, 20, 24, 32};
    if ((rate && rate != si.sample_rate) || (ssc && DEPTH[ssc] != si.bps) || (ca < 8 ? ca + 1 : 2u) != si.channels) return false;
    uint8_t crc = 0;
    for (uint64_t i = p; i < q; i++) crc = crc8_byte(crc, d[i]);
    if (crc != d[q]) return false;
    h->blocksize = bs;
    h->header_bytes = (uint32_t)(q + 1 - p);
    return true;
}

// The frame table.  rows[i].nbytes runs from the frame's header to the next frame's (the CRC-16 included); the last frame
// ends at the end of the data.  *total = the samples the frames hold (STREAMINFO's count when it gives one and it is smaller).
// first_sample counts from the first frame of the file; *base = the stream position that frame's header codes (0 unless the
// file was cut out of a longer stream), which the frame decoder adds when it compares a variable-block-size header.
inline int index_frames(const uint8_t* d, uint64_t n, const StreamInfo& si, bool verified, std::vector<FrameRow>* rows,
                        uint64_t* total, uint64_t* base, bool* last_crc_ok = nullptr) {
    rows->clear();
    *total = 0;
    *base = 0;
    if (last_crc_ok) *last_crc_ok = false;
    uint64_t p = si.first_frame, sample = 0, fixed_bs = 0, expect = 0;
    bool variable = false;
    FrameHeader h;
    if (p >= n || !parse_frame_header(d, n, p, si, &h)) return INDEX_NO_FRAMES;
    variable = h.variable;
    fixed_bs = si.min_block == si.max_block && si.min_block ? si.min_block : h.blocksize;
    const uint64_t first_number = h.number;
    *base = variable ? h.number : h.number * fixed_bs;
    expect = h.number;
    for (;;) {
        // frame at p with header h; find where it ends
        const uint64_t next_sample = sample + h.blocksize;
        expect = variable ? *base + next_sample : expect + 1;
        uint64_t from = p + (!verified && si.min_frame > h.header_bytes ? si.min_frame : h.header_bytes + 1);
        uint64_t end = n;
        FrameHeader nh;
        bool found = false;
        uint16_t crc = 0;
        uint64_t crc_to = p;  // crc covers [p, crc_to)
        while (from < n) {
            const uint8_t* m = (const uint8_t*)memchr(d + from, 0xFF, (size_t)(n - from));
            if (!m) break;
            const uint64_t cand = (uint64_t)(m - d);
            from = cand + 1;
            if (!parse_frame_header(d, n, cand, si, &nh) || nh.variable != variable || nh.number != expect) continue;
            if (verified) {
                if (cand < p + 2) continue;
                crc = crc16_update(crc, d + crc_to, (size_t)(cand - 2 - crc_to));
                crc_to = cand - 2;
                if (crc != (((uint16_t)d[cand - 2] << 8) | d[cand - 1])) continue;
            }
            end = cand;
            found = true;
            break;
        }
        if (!found && verified && last_crc_ok && n >= p + 2 + h.header_bytes) {
            crc = crc16_update(crc, d + crc_to, (size_t)(n - 2 - crc_to));
            *last_crc_ok = crc == (((uint16_t)d[n - 2] << 8) | d[n - 1]);
        }
        rows->push_back(FrameRow{p, end - p, sample, h.blocksize});
        sample = next_sample;
        if (!found) break;
        if (!variable && h.blocksize != fixed_bs) {
            // a short block in a fixed-block-size stream is the last one; what follows cannot be placed
            break;
        }
        p = end;
        h = nh;
        if (!variable) sample = (h.number - first_number) * fixed_bs;
    }
    *total = si.total && si.total < sample ? si.total : sample;
    return si.total && sample < si.total ? INDEX_TRUNCATED : INDEX_OK;  // frames are missing: the table is still filled
}

}  // namespace flac
