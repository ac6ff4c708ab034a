// Stand-alone host build of the FLAC path: flac_index.hpp (STREAMINFO, frame table) + flac_frame.hpp (the frame decoder the
// device runs, one lane per frame) on the CPU.  No GPU, no libblissgpu.so.
//
//   test_flac FILE [OUT.pcm]           decode FILE the way blissgpu_analyze_batch_flac does (fast index, end-position check,
//                                      verified index on a mismatch) and print key=value lines: the STREAMINFO fields, both
//                                      frame tables, the status and the MD5 of the samples (as FLAC defines it).
//   test_flac --fuzz SEED COUNT M FILE..  every FILE as it is, then COUNT seeded mutations spread over the first M files (byte
//                                      flips, truncations, duplicated ranges).  Every input has to end in a status; the buffers
//                                      are exact-size so that a sanitizer build sees any load or store outside them.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../bliss-rs_amd/csrc/flac_frame.hpp"
#include "../../bliss-rs_amd/csrc/flac_index.hpp"

namespace {

struct Md5 {
    uint32_t a = 0x67452301, b = 0xefcdab89, c = 0x98badcfe, d = 0x10325476;
    uint64_t len = 0;
    uint8_t buf[64];
    size_t fill = 0;
    void block(const uint8_t* p) {
        static const uint32_t K[64] = {
            0xd76aa478, 0xe8c7b756, 0x242070db, 0xc1bdceee, 0xf57c0faf, 0x4787c62a, 0xa8304613, 0xfd469501, 0x698098d8, 0x8b44f7af, 0xffff5bb1,
            0x895cd7be, 0x6b901122, 0xfd987193, 0xa679438e, 0x49b40821, 0xf61e2562, 0xc040b340, 0x265e5a51, 0xe9b6c7aa, 0xd62f105d, 0x02441453,
            0xd8a1e681, 0xe7d3fbc8, 0x21e1cde6, 0xc33707d6, 0xf4d50d87, 0x455a14ed, 0xa9e3e905, 0xfcefa3f8, 0x676f02d9, 0x8d2a4c8a, 0xfffa3942,
            0x8771f681, 0x6d9d6122, 0xfde5380c, 0xa4beea44, 0x4bdecfa9, 0xf6bb4b60, 0xbebfbc70, 0x289b7ec6, 0xeaa127fa, 0xd4ef3085, 0x04881d05,
            0xd9d4d039, 0xe6db99e5, 0x1fa27cf8, 0xc4ac5665, 0xf4292244, 0x432aff97, 0xab9423a7, 0xfc93a039, 0x655b59c3, 0x8f0ccc92, 0xffeff47d,
            0x85845dd1, 0x6fa87e4f, 0xfe2ce6e0, 0xa3014314, 0x4e0811a1, 0xf7537e82, 0xbd3af235, 0x2ad7d2bb, 0xeb86d391};
        static const int S[64] = {7, 12, 17, 22, 7, 12, 17, 22, 7, 12, 17, 22, 7, 12, 17, 22, 5, 9,  14, 20, 5, 9,  14, 20, 5, 9,  14, 20, 5, 9,  14, 20,
                                  4, 11, 16, 23, 4, 11, 16, 23, 4, 11, 16, 23, 4, 11, 16, 23, 6, 10, 15, 21, 6, 10, 15, 21, 6, 10, 15, 21, 6, 10, 15, 21};
        uint32_t m[16];
        for (int i = 0; i < 16; i++) m[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 | (uint32_t)p[4 * i + 3] << 24;
        uint32_t A = a, B = b, C = c, D = d;
        for (int i = 0; i < 64; i++) {
            uint32_t f;
            int g;
            if (i < 16) { f = (B & C) | (~B & D); g = i; }
            else if (i < 32) { f = (D & B) | (~D & C); g = (5 * i + 1) & 15; }
            else if (i < 48) { f = B ^ C ^ D; g = (3 * i + 5) & 15; }
            else { f = C ^ (B | ~D); g = (7 * i) & 15; }
            f += A + K[i] + m[g];
            A = D;
            D = C;
            C = B;
            B += (f << S[i]) | (f >> (32 - S[i]));
        }
        a += A; b += B; c += C; d += D;
    }
    void update(const uint8_t* p, size_t n) {
        len += n;
        while (n) {
            const size_t k = n < 64 - fill ? n : 64 - fill;
            memcpy(buf + fill, p, k);
            fill += k; p += k; n -= k;
            if (fill == 64) { block(buf); fill = 0; }
        }
    }
    std::string hex() {
        const uint64_t bits = len * 8;
        const uint8_t one = 0x80, zero = 0;
        update(&one, 1);
        while (fill != 56) update(&zero, 1);
        uint8_t l[8];
        for (int i = 0; i < 8; i++) l[i] = (uint8_t)(bits >> (8 * i));
        update(l, 8);
        char out[33];
        const uint32_t w[4] = {a, b, c, d};
        for (int i = 0; i < 16; i++) snprintf(out + 2 * i, 3, "%02x", (w[i / 4] >> (8 * (i % 4))) & 0xFF);
        return out;
    }
};

struct Decoded {
    int status = 0;         // 0, or 100 + IndexError, or 200 + the first bad frame's FrameStatus, or 300 = end-position mismatch
    bool slow = false;      // took the verified road
    flac::StreamInfo si;
    uint64_t total = 0, base = 0;
    std::vector<uint8_t> pcm;  // exactly total x channels x (2 or 4) bytes
    std::vector<flac::FrameRow> rows;
};

// frames of one table into d.pcm; 0 or the status as above
int decode_rows(const uint8_t* padded, uint64_t n, Decoded& d) {
    const size_t width = d.si.bps > 16 ? 4 : 2;
    d.pcm.assign((size_t)(d.total * d.si.channels * width), 0);
    flac::HostWin win;
    for (size_t i = 0; i < d.rows.size(); i++) {
        const flac::FrameRow& r = d.rows[i];
        uint64_t end = 0;
        const int st = flac::decode_frame(padded, n, r.offset, r.nbytes, r.first_sample, (uint32_t)r.blocksize, d.si.channels, d.si.bps,
                                          d.total, d.base, d.pcm.data(), win, &end);
        if (st != flac::FRAME_OK) return 200 + st;
        const bool last = i + 1 == d.rows.size();   // (trailing bytes may follow the last frame)
        if (last ? end + 2 > r.offset + r.nbytes : end + 2 != r.offset + r.nbytes) return 300;
    }
    return 0;
}

Decoded decode_file(const std::vector<uint8_t>& file) {
    Decoded d;
    const uint64_t n = file.size();
    // the decoder's contract: 16 readable bytes behind the file, and not one more
    std::vector<uint8_t> padded(file.size() + flac::FILE_PAD, 0);
    if (n) memcpy(padded.data(), file.data(), n);
    int rc = flac::stream_info(padded.data(), n, &d.si);
    if (rc) { d.status = 100 + rc; return d; }
    if (d.si.bps < 4 || d.si.bps > 24) { d.status = 200 + flac::FRAME_UNSUPPORTED_DEPTH; return d; }
    for (int verified = 0; verified < 2; verified++) {
        d.slow = verified;
        rc = flac::index_frames(padded.data(), n, d.si, verified, &d.rows, &d.total, &d.base);
        d.status = rc ? 100 + rc : decode_rows(padded.data(), n, d);
        if (d.status == 0) break;
    }
    if (d.status) d.pcm.clear();
    return d;
}

std::string stream_md5(const Decoded& d) {
    Md5 m;
    const uint32_t bytes = (d.si.bps + 7) / 8, shift = (d.si.bps > 16 ? 32 : 16) - d.si.bps;
    const size_t count = (size_t)(d.total * d.si.channels);
    std::vector<uint8_t> le(count * bytes);
    for (size_t i = 0; i < count; i++) {
        int32_t v;
        if (d.si.bps > 16) { memcpy(&v, d.pcm.data() + 4 * i, 4); }
        else { int16_t s; memcpy(&s, d.pcm.data() + 2 * i, 2); v = s; }
        v >>= shift;
        for (uint32_t k = 0; k < bytes; k++) le[i * bytes + k] = (uint8_t)((uint32_t)v >> (8 * k));
    }
    m.update(le.data(), le.size());
    return m.hex();
}

bool read_file(const char* path, std::vector<uint8_t>* out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    size_t k;
    out->clear();
    while ((k = fread(buf, 1, sizeof(buf), f)) > 0) out->insert(out->end(), buf, buf + k);
    fclose(f);
    return true;
}

void print_table(const char* name, const std::vector<flac::FrameRow>& rows) {
    printf("%s=", name);
    for (size_t i = 0; i < rows.size(); i++)
        printf("%s%llu:%llu:%llu:%llu", i ? "," : "", (unsigned long long)rows[i].offset, (unsigned long long)rows[i].nbytes,
               (unsigned long long)rows[i].first_sample, (unsigned long long)rows[i].blocksize);
    printf("\n");
}

int fuzz(int argc, char** argv) {
    uint64_t rng = strtoull(argv[2], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1;
    const long count = strtol(argv[3], nullptr, 10);
    auto next = [&rng]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    const size_t n_mutate = (size_t)strtoul(argv[4], nullptr, 10);
    std::vector<std::vector<uint8_t>> files;
    for (int i = 5; i < argc; i++) {
        files.emplace_back();
        if (!read_file(argv[i], &files.back())) { fprintf(stderr, "cannot read %s\n", argv[i]); return 2; }
    }
    if (files.empty() || n_mutate == 0 || n_mutate > files.size()) return 2;
    long ok = 0, bad = 0;
    for (const auto& f : files) (decode_file(f).status ? bad : ok)++;
    for (long it = 0; it < count; it++) {
        std::vector<uint8_t> m = files[(size_t)it % n_mutate];
        if (m.empty()) continue;
        const int kind = (int)(next() % 3);
        if (kind == 0) {  // byte flips
            const int flips = 1 + (int)(next() % 4);
            for (int k = 0; k < flips; k++) m[(size_t)(next() % m.size())] ^= (uint8_t)(1u << (next() % 8));
        } else if (kind == 1) {  // truncation
            m.resize((size_t)(next() % m.size()));
        } else {  // a range duplicated in place
            const size_t a = (size_t)(next() % m.size()), len = 1 + (size_t)(next() % 64);
            const size_t b = a + len < m.size() ? a + len : m.size();
            std::vector<uint8_t> piece(m.begin() + (long)a, m.begin() + (long)b);
            m.insert(m.begin() + (long)b, piece.begin(), piece.end());
        }
        (decode_file(m).status ? bad : ok)++;
    }
    printf("inputs=%ld decoded=%ld refused=%ld\n", ok + bad, ok, bad);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 6 && !strcmp(argv[1], "--fuzz")) return fuzz(argc, argv);
    if (argc < 2) { fprintf(stderr, "usage: test_flac FILE [OUT.pcm] | --fuzz SEED COUNT M FILE...\n"); return 2; }
    std::vector<uint8_t> file;
    if (!read_file(argv[1], &file)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    Decoded d = decode_file(file);
    printf("status=%d\nslow=%d\n", d.status, (int)d.slow);
    if (d.status >= 100 && d.status < 200) return 0;
    char md5[33];
    for (int i = 0; i < 16; i++) snprintf(md5 + 2 * i, 3, "%02x", d.si.md5[i]);
    printf("rate=%u\nchannels=%u\nbps=%u\nstream_total=%llu\nmin_block=%u\nmax_block=%u\nmin_frame=%u\nfirst_frame=%llu\nstream_md5=%s\n",
           d.si.sample_rate, d.si.channels, d.si.bps, (unsigned long long)d.si.total, d.si.min_block, d.si.max_block, d.si.min_frame,
           (unsigned long long)d.si.first_frame, md5);
    std::vector<uint8_t> padded(file.size() + flac::FILE_PAD, 0);
    memcpy(padded.data(), file.data(), file.size());
    std::vector<flac::FrameRow> rows;
    uint64_t total = 0, base = 0;
    int rc = flac::index_frames(padded.data(), file.size(), d.si, false, &rows, &total, &base);
    printf("fast_rc=%d\n", rc);
    print_table("fast", rows);
    bool last_crc_ok = false;
    rc = flac::index_frames(padded.data(), file.size(), d.si, true, &rows, &total, &base, &last_crc_ok);
    printf("verified_rc=%d\nlast_crc_ok=%d\n", rc, (int)last_crc_ok);
    print_table("verified", rows);
    if (d.status == 0) {
        printf("total=%llu\nmd5=%s\n", (unsigned long long)d.total, stream_md5(d).c_str());
        if (argc > 2) {
            FILE* f = fopen(argv[2], "wb");
            if (!f || fwrite(d.pcm.data(), 1, d.pcm.size(), f) != d.pcm.size()) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
            fclose(f);
        }
    }
    return 0;
}
