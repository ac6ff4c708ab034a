// Stand-alone host build of the FLAC checks: flac_verify.hpp (the frame CRC-16 as the 64 lanes of flac_crc_kernel compute it,
// the MD5 as flac_md5_kernel computes it) on the CPU, over flac_index.hpp + flac_frame.hpp.  No GPU, no libblissgpu.so.
// Every buffer is exact-size -- the file plus the 16 bytes of padding the loads are promised, the PCM exactly total x channels
// samples -- so that a sanitizer build sees any load or store outside them.
//
//   test_flac_verify --crc SEED               the lane-decomposed CRC against the byte-serial one: every start offset 0..7 and
//                                             every length 1..1100 of seeded random bytes; the combine identity at every split
//                                             of a 300-byte message; leading zeros; the byte step against the bit-by-bit form
//   test_flac_verify --frames FILE ROWS       ROWS = off:len,off:len,...: each frame's remainder over its bytes INCLUDING the
//                                             CRC field (0 for a sound frame), lane by lane
//   test_flac_verify --verdict FILE..         every FILE the way blissgpu_flac_verify_batch treats it: name flags first_bad md5
//   test_flac_verify --md5-strings            the seven strings of RFC 1321's test suite: one digest per line
//   test_flac_verify --md5-file BLOB          messages of 0, 1, 2, .. bytes cut one behind the other from BLOB: one digest each
//   test_flac_verify --md5-pcm FILE:BPS ..    FILE = a PCM region (int16 up to 16 bits, int32 above): the FLAC message's digest
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../bliss-rs_amd/csrc/flac_frame.hpp"
#include "../../bliss-rs_amd/csrc/flac_index.hpp"
#include "../../bliss-rs_amd/csrc/flac_verify.hpp"

namespace {

bool read_file(const char* path, std::vector<uint8_t>* out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    out->clear();
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out->insert(out->end(), buf, buf + n);
    fclose(f);
    return true;
}

std::string hex(const uint32_t* d) {
    char out[33];
    for (int i = 0; i < 16; i++) snprintf(out + 2 * i, 3, "%02x", (d[i / 4] >> (8 * (i % 4))) & 0xFF);
    return out;
}

uint64_t rng_state;
uint32_t rng() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

uint32_t crc_bits(const uint8_t* p, size_t n) {
    uint32_t c = 0;
    for (size_t i = 0; i < n; i++) c = flac::crc16_bitwise(c, p[i]);
    return c;
}

int run_crc(uint64_t seed) {
    rng_state = seed * 2 + 1;
    uint64_t cases = 0;
    // the table-free byte step is the definition: every register value, a spread of bytes; every byte, a spread of registers
    for (uint32_t c = 0; c < 65536; c++)
        for (uint32_t b : {0u, 1u, 0x80u, 0xFFu, 0x5Au, c & 0xFFu})
            if (flac::crc16_byte(c, b) != flac::crc16_bitwise(c, b)) { printf("byte step differs at c=%u b=%u\n", c, b); return 1; }
    for (uint32_t b = 0; b < 256; b++)
        for (uint32_t c : {0u, 1u, 0x8000u, 0xFFFFu, 0x1234u})
            if (flac::crc16_byte(c, b) != flac::crc16_bitwise(c, b)) { printf("byte step differs at c=%u b=%u\n", c, b); return 1; }
    // lanes against the serial form: one partial word, 63 / 64 / 65 words, two full rounds plus one byte are all in 1..1100
    for (uint32_t off = 0; off < 8; off++)
        for (uint32_t len = 1; len <= 1100; len++) {
            const uint64_t n = (uint64_t)off + len;  // the "file" ends with the frame
            std::vector<uint8_t> file(n + flac::FILE_PAD);
            for (auto& b : file) b = (uint8_t)rng();  // (the padding and the bytes in front are NOT zero: they must not count)
            const uint32_t want = crc_bits(file.data() + off, len);
            if (flac::crc16_serial(file.data() + off, len) != want) { printf("serial differs off=%u len=%u\n", off, len); return 1; }
            const uint32_t got = flac::crc16_lanes(file.data(), off, n);
            if (got != want) { printf("lanes differ off=%u len=%u: %04x != %04x\n", off, len, got, want); return 1; }
            cases++;
        }
    // a frame in the middle of a file: bytes behind its end must not count either
    for (uint32_t k = 0; k < 2000; k++) {
        const uint32_t off = rng() % 3000, len = 1 + rng() % 2500, behind = rng() % 40;
        std::vector<uint8_t> file((size_t)off + len + behind + flac::FILE_PAD);
        for (auto& b : file) b = (uint8_t)rng();
        if (flac::crc16_lanes(file.data(), off, (uint64_t)off + len) != crc_bits(file.data() + off, len)) { printf("lanes differ off=%u len=%u\n", off, len); return 1; }
        cases++;
    }
    // crc(A || B) = crc(A) x^(8 |B|) mod P xor crc(B), at every split point of a 300-byte message
    std::vector<uint8_t> msg(300);
    for (auto& b : msg) b = (uint8_t)rng();
    const uint32_t whole = crc_bits(msg.data(), msg.size());
    for (size_t cut = 0; cut <= msg.size(); cut++) {
        const uint32_t a = crc_bits(msg.data(), cut), b = crc_bits(msg.data() + cut, msg.size() - cut);
        if (flac::crc16_combine(a, b, msg.size() - cut) != whole) { printf("combine differs at %zu\n", cut); return 1; }
        cases++;
    }
    // leading zeros change nothing
    for (size_t z = 0; z <= 70; z++) {
        std::vector<uint8_t> m(z, 0);
        m.insert(m.end(), msg.begin(), msg.end());
        if (crc_bits(m.data(), m.size()) != whole || flac::crc16_serial(m.data(), m.size()) != whole) { printf("leading zeros count at %zu\n", z); return 1; }
        cases++;
    }
    // x^(8 n) mod P is n zero bytes behind a one
    uint32_t c = 1;
    for (uint64_t n = 0; n <= 2000; n++) {
        if (flac::crc16_xpow8(n) != c) { printf("xpow8 differs at %llu\n", (unsigned long long)n); return 1; }
        c = flac::crc16_bitwise(c, 0);
    }
    if (flac::CRC16_X_ROUND != flac::crc16_xpow8(512)) return 1;
    printf("crc_cases=%llu\n", (unsigned long long)cases);
    return 0;
}

int run_frames(const char* path, const char* rows) {
    std::vector<uint8_t> file;
    if (!read_file(path, &file)) return 2;
    const uint64_t n = file.size();
    file.resize(n + flac::FILE_PAD, 0xA5);
    uint64_t frames = 0, nonzero = 0;
    for (const char* p = rows; *p;) {
        char* e;
        const uint64_t off = strtoull(p, &e, 10);
        const uint64_t len = strtoull(e + 1, &e, 10);
        p = *e ? e + 1 : e;
        if (off > n || len > n - off || len < 3) return 3;
        frames++;
        const uint32_t rem = flac::crc16_lanes(file.data(), off, off + len);
        const uint32_t body = flac::crc16_lanes(file.data(), off, off + len - 2);
        const uint32_t stored = (uint32_t)file[off + len - 2] << 8 | file[off + len - 1];
        if (rem != 0 || body != stored) nonzero++;
    }
    printf("frames=%llu\nnonzero=%llu\n", (unsigned long long)frames, (unsigned long long)nonzero);
    return 0;
}

// flags as include/blissgpu.h names them
constexpr uint32_t BAD_STREAM = 1, BAD_CRC16 = 2, BAD_MD5 = 4, MD5_UNCHECKED = 8;

void verdict(const char* path) {
    std::vector<uint8_t> raw;
    uint32_t flags = MD5_UNCHECKED, first_bad = 0xFFFFFFFFu;
    uint32_t digest[4] = {0, 0, 0, 0};
    bool computed = false;
    const char* name = strrchr(path, '/') ? strrchr(path, '/') + 1 : path;
    if (!read_file(path, &raw)) { printf("%s %u %u -\n", name, BAD_STREAM | MD5_UNCHECKED, first_bad); return; }
    const uint64_t n = raw.size();
    std::vector<uint8_t> file(n + flac::FILE_PAD, 0);
    if (n) memcpy(file.data(), raw.data(), n);
    flac::StreamInfo si;
    bool sound = flac::stream_info(file.data(), n, &si) == 0 && si.bps >= 4 && si.bps <= 24;
    std::vector<flac::FrameRow> rows;
    std::vector<uint64_t> ends;
    std::vector<uint8_t> pcm;
    uint64_t total = 0, base = 0;
    if (sound) {
        sound = false;
        for (int verified = 0; verified < 2 && !sound; verified++) {
            if (flac::index_frames(file.data(), n, si, verified != 0, &rows, &total, &base)) continue;
            pcm.assign((size_t)(total * si.channels * (si.bps > 16 ? 4 : 2)), 0);
            ends.assign(rows.size(), 0);
            flac::HostWin win;
            sound = true;
            for (size_t i = 0; i < rows.size() && sound; i++) {
                const flac::FrameRow& r = rows[i];
                const int st = flac::decode_frame(file.data(), n, r.offset, r.nbytes, r.first_sample, (uint32_t)r.blocksize, si.channels, si.bps, total,
                                                  base, pcm.data(), win, &ends[i]);
                const bool last = i + 1 == rows.size();
                sound = st == flac::FRAME_OK && (last ? ends[i] + 2 <= r.offset + r.nbytes : ends[i] + 2 == r.offset + r.nbytes);
            }
        }
    }
    if (!sound) flags |= BAD_STREAM;
    if (sound) {
        for (size_t i = 0; i < rows.size(); i++) {
            const uint64_t stop = ends[i];
            const uint32_t c = flac::crc16_lanes(file.data(), rows[i].offset, stop);
            if (c != ((uint32_t)file[stop] << 8 | file[stop + 1])) {
                flags |= BAD_CRC16;
                if (first_bad == 0xFFFFFFFFu) first_bad = (uint32_t)i;
            }
        }
        static const uint8_t zero[16] = {0};
        if (!(flags & BAD_CRC16) && memcmp(si.md5, zero, 16) && base == 0 && (si.total == 0 || si.total == total)) {
            // (an exact-size, 4-byte aligned copy of the region)
            std::vector<uint32_t> region((pcm.size() + 3) / 4);
            if (!pcm.empty()) memcpy(region.data(), pcm.data(), pcm.size());
            flac::md5_pcm(region.data(), total * si.channels, si.bps, digest);
            computed = true;
            flags &= ~MD5_UNCHECKED;
            if (memcmp(digest, si.md5, 16)) flags |= BAD_MD5;
        }
    }
    printf("%s %u %u %s\n", name, flags, first_bad, computed ? hex(digest).c_str() : "-");
}

int run_md5_strings() {
    const char* suite[7] = {"", "a", "abc", "message digest", "abcdefghijklmnopqrstuvwxyz",
                            "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789",
                            "12345678901234567890123456789012345678901234567890123456789012345678901234567890"};
    for (const char* s : suite) {
        const size_t n = strlen(s);
        std::vector<uint8_t> m(s, s + n);  // exact size
        uint32_t d[4];
        flac::md5_run(n, flac::Md5Bytes{m.data(), n}, d);
        printf("%s\n", hex(d).c_str());
    }
    return 0;
}

int run_md5_file(const char* path) {
    std::vector<uint8_t> blob;
    if (!read_file(path, &blob)) return 2;
    size_t pos = 0;
    for (size_t n = 0; pos + n <= blob.size(); pos += n, n++) {
        std::vector<uint8_t> m(blob.begin() + pos, blob.begin() + pos + n);
        uint32_t d[4];
        flac::md5_run(n, flac::Md5Bytes{m.data(), n}, d);
        printf("%s\n", hex(d).c_str());
    }
    return 0;
}

int run_md5_pcm(int argc, char** argv) {
    for (int i = 0; i < argc; i++) {
        std::string spec = argv[i];
        const size_t colon = spec.rfind(':');
        if (colon == std::string::npos) return 2;
        const uint32_t bps = (uint32_t)atoi(spec.c_str() + colon + 1);
        std::vector<uint8_t> raw;
        if (!read_file(spec.substr(0, colon).c_str(), &raw) || bps < 4 || bps > 24) return 2;
        const size_t esz = bps > 16 ? 4 : 2;
        std::vector<uint8_t> exact(raw);  // the allocation ends with the last element
        uint32_t d[4];
        flac::md5_pcm(exact.data(), raw.size() / esz, bps, d);
        printf("%s\n", hex(d).c_str());
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 3 && !strcmp(argv[1], "--crc")) return run_crc(strtoull(argv[2], nullptr, 10));
    if (argc >= 4 && !strcmp(argv[1], "--frames")) return run_frames(argv[2], argv[3]);
    if (argc >= 2 && !strcmp(argv[1], "--verdict")) {
        for (int i = 2; i < argc; i++) verdict(argv[i]);
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "--md5-strings")) return run_md5_strings();
    if (argc >= 3 && !strcmp(argv[1], "--md5-file")) return run_md5_file(argv[2]);
    if (argc >= 2 && !strcmp(argv[1], "--md5-pcm")) return run_md5_pcm(argc - 2, argv + 2);
    fprintf(stderr, "usage: see the head of tests/cpp/test_flac_verify.cpp\n");
    return 64;
}
