// bliss_audio.hpp -- C++17 host-side mirror of the bliss-rs interface for the analysis hot path,
// implemented on top of the C ABI in include/blissgpu.h (header-only; link with -lblissgpu).
//
// The reference is a Rust crate and this image has no Rust toolchain, so this header is the compiled
// host layer that is tested here; the Rust binding a bliss-rs maintainer would add is in
// INTEGRATION.md.  Names, argument meaning and error behaviour follow the reference:
//
//   bliss::Song::analyze / analyze_with_options      src/song/mod.rs:403-508
//   bliss::Analysis, AnalysisIndex, FeaturesVersion  src/song/mod.rs:102-371, src/lib.rs:151-187
//   bliss::BlissError {Decoding,Analysis,Provider}   src/lib.rs:236-252
//   bliss::Decoder (decode / song_from_path / analyze_paths)   src/song/decoder.rs:115-333
//   bliss::FlacDecoder: .flac files handed to the device COMPRESSED (blissgpu_analyze_batch_flac); no CPU entropy decoding
//   bliss::euclidean_distance / cosine_distance / mahalanobis_distance   src/playlist.rs:65-142
#pragma once
#include <algorithm>
#include <array>
#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <map>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <variant>
#include <vector>

#include "../../include/blissgpu.h"

namespace bliss {

constexpr uint32_t SAMPLE_RATE = 22050;  // src/lib.rs:140
constexpr uint16_t CHANNELS = 1;         // src/lib.rs:137

// ---- BlissError (src/lib.rs:236-252): value-returned on the analysis path, thrown here ----
struct BlissError : std::runtime_error {
    enum class Kind { DecodingError, AnalysisError, ProviderError } kind;
    std::string message;
    BlissError(Kind k, std::string m) : std::runtime_error(prefix(k) + m), kind(k), message(std::move(m)) {}
    static std::string prefix(Kind k) {
        switch (k) {
            case Kind::DecodingError: return "error happened while decoding file - ";
            case Kind::AnalysisError: return "error happened while analyzing file - ";
            default: return "error happened with the music library provider - ";
        }
    }
    bool operator==(const BlissError& o) const { return kind == o.kind && message == o.message; }
};
inline BlissError AnalysisError(std::string m) { return BlissError(BlissError::Kind::AnalysisError, std::move(m)); }
inline BlissError DecodingError(std::string m) { return BlissError(BlissError::Kind::DecodingError, std::move(m)); }
inline BlissError ProviderError(std::string m) { return BlissError(BlissError::Kind::ProviderError, std::move(m)); }

// a failure of the GPU library itself (no device, HIP error): not a BlissError, there is no CPU path
struct GpuError : std::runtime_error {
    int code;
    GpuError(int c) : std::runtime_error(std::string("blissgpu: ") + blissgpu_strerror(c) + " (" + blissgpu_last_error() + ")"), code(c) {}
};
inline void check(int rc) { if (rc != BLISSGPU_OK) throw GpuError(rc); }

// ---- FeaturesVersion (src/lib.rs:151-187) ----
enum class FeaturesVersion : uint16_t { Version1 = 1, Version2 = 2 };
constexpr FeaturesVersion LATEST = FeaturesVersion::Version2;
constexpr size_t feature_count(FeaturesVersion v) { return v == FeaturesVersion::Version2 ? 23 : 20; }
constexpr size_t NUMBER_FEATURES = feature_count(LATEST);  // src/song/mod.rs:222
inline FeaturesVersion features_version_try_from(uint16_t v) {
    if (v == 1 || v == 2) return static_cast<FeaturesVersion>(v);
    throw ProviderError("This features' version (" + std::to_string(v) + ") does not exist");
}
inline std::vector<float> feature_weights(FeaturesVersion v) {  // row-major d x d
    std::vector<float> m(feature_count(v) * feature_count(v));
    check(blissgpu_feature_weights(static_cast<uint32_t>(v), m.data()));
    return m;
}

// ---- AnalysisIndex (src/song/mod.rs:102-156) ----
enum class AnalysisIndex : size_t {
    Tempo, Zcr, MeanSpectralCentroid, StdDeviationSpectralCentroid, MeanSpectralRolloff, StdDeviationSpectralRolloff,
    MeanSpectralFlatness, StdDeviationSpectralFlatness, MeanLoudness, StdDeviationLoudness,
    Chroma1, Chroma2, Chroma3, Chroma4, Chroma5, Chroma6, Chroma7, Chroma8, Chroma9, Chroma10, Chroma11, Chroma12, Chroma13
};

struct AnalysisOptions {  // src/song/mod.rs:248-269
    FeaturesVersion features_version = LATEST;
    size_t number_cores = 1;  // kept for interface parity; the batch is scheduled on the GPU
};

// ---- distances (src/playlist.rs:65-79, 129-142) ----
inline float distance(const std::vector<float>& a, const std::vector<float>& b, int metric, const float* m = nullptr) {
    if (a.size() != b.size()) throw std::invalid_argument("vectors must have the same length");
    float out = 0.0f;
    check(blissgpu_distance(a.data(), b.data(), static_cast<uint32_t>(a.size()), metric, m, &out));
    return out;
}
inline float euclidean_distance(const std::vector<float>& a, const std::vector<float>& b) { return distance(a, b, BLISSGPU_METRIC_EUCLIDEAN); }
inline float cosine_distance(const std::vector<float>& a, const std::vector<float>& b) { return distance(a, b, BLISSGPU_METRIC_COSINE); }
inline float mahalanobis_distance(const std::vector<float>& a, const std::vector<float>& b, const std::vector<float>& m) {
    return distance(a, b, BLISSGPU_METRIC_MAHALANOBIS, m.data());
}
using DistanceFn = std::function<float(const std::vector<float>&, const std::vector<float>&)>;
inline DistanceFn mahalanobis_distance_builder(std::vector<float> m) {
    return [m = std::move(m)](const std::vector<float>& a, const std::vector<float>& b) { return mahalanobis_distance(a, b, m); };
}
inline DistanceFn distance_metric(FeaturesVersion v) { return mahalanobis_distance_builder(feature_weights(v)); }  // src/lib.rs:176-178

// ---- Analysis (src/song/mod.rs:238-371) ----
class Analysis {
  public:
    std::vector<float> internal_analysis;
    FeaturesVersion features_version = LATEST;
    Analysis() = default;
    Analysis(std::vector<float> analysis, FeaturesVersion v) : internal_analysis(std::move(analysis)), features_version(v) {
        if (internal_analysis.size() != feature_count(v))
            throw ProviderError("Feature count " + std::to_string(internal_analysis.size()) +
                                " does not match the expected version feature count " + std::to_string(feature_count(v)));
    }
    const std::vector<float>& as_vec() const { return internal_analysis; }
    float operator[](AnalysisIndex i) const {
        if (features_version != LATEST) throw std::logic_error("Tried to index features with incompatible indexes");
        return internal_analysis[static_cast<size_t>(i)];
    }
    bool operator==(const Analysis& o) const { return features_version == o.features_version && internal_analysis == o.internal_analysis; }
    // default distance for the FeaturesVersion; the reference panics on mismatched versions (:364-370)
    float distance(const Analysis& other) const {
        if (features_version != other.features_version) throw std::logic_error("Mismatched features version between two songs or analysis");
        return distance_metric(features_version)(internal_analysis, other.internal_analysis);
    }
};

template <typename T>
using BlissResult = std::variant<T, BlissError>;

// Bulk Song::analyze_with_options over songs already decoded to mono 22 050 Hz f32 (one GPU batch).
inline std::vector<BlissResult<Analysis>> analyze_batch(const std::vector<std::vector<float>>& songs, const AnalysisOptions& opt = {}) {
    const uint32_t n = static_cast<uint32_t>(songs.size());
    const size_t d = feature_count(opt.features_version);
    std::vector<uint64_t> off(n), len(n);
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) { off[i] = total; len[i] = songs[i].size(); total += len[i]; }
    std::vector<float> pcm(total ? total : 1);
    for (uint32_t i = 0; i < n; i++) std::copy(songs[i].begin(), songs[i].end(), pcm.begin() + off[i]);
    std::vector<float> out(n * d);
    std::vector<int32_t> status(n);
    if (n) check(blissgpu_analyze_batch(pcm.data(), off.data(), len.data(), n, static_cast<uint32_t>(opt.features_version), out.data(), status.data()));
    std::vector<BlissResult<Analysis>> res;
    res.reserve(n);
    for (uint32_t i = 0; i < n; i++) {
        if (status[i] == BLISSGPU_SONG_OK) res.emplace_back(Analysis(std::vector<float>(out.begin() + i * d, out.begin() + (i + 1) * d), opt.features_version));
        else if (status[i] == BLISSGPU_SONG_TOO_SHORT) res.emplace_back(AnalysisError("empty or too short song."));
        else res.emplace_back(AnalysisError("analysis failed with status " + std::to_string(status[i])));
    }
    return res;
}

// Same for decoders that deliver s16 mono 22 050 Hz PCM: 2 bytes per sample over PCIe, widened on the device exactly
// like FFmpeg's s16 -> flt conversion (sample / 32768, src/song/decoder/ffmpeg.rs:36-109).
inline std::vector<BlissResult<Analysis>> analyze_batch(const std::vector<std::vector<int16_t>>& songs, const AnalysisOptions& opt = {}) {
    const uint32_t n = static_cast<uint32_t>(songs.size());
    const size_t d = feature_count(opt.features_version);
    std::vector<uint64_t> off(n), len(n);
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) { off[i] = total; len[i] = songs[i].size(); total += len[i]; }
    std::vector<int16_t> pcm(total ? total : 1);
    for (uint32_t i = 0; i < n; i++) std::copy(songs[i].begin(), songs[i].end(), pcm.begin() + off[i]);
    std::vector<float> out(n * d);
    std::vector<int32_t> status(n);
    if (n) check(blissgpu_analyze_batch_s16(pcm.data(), off.data(), len.data(), n, static_cast<uint32_t>(opt.features_version), out.data(), status.data()));
    std::vector<BlissResult<Analysis>> res;
    res.reserve(n);
    for (uint32_t i = 0; i < n; i++) {
        if (status[i] == BLISSGPU_SONG_OK) res.emplace_back(Analysis(std::vector<float>(out.begin() + i * d, out.begin() + (i + 1) * d), opt.features_version));
        else res.emplace_back(AnalysisError("empty or too short song."));
    }
    return res;
}

// ---- Song (src/song/mod.rs:45-76, 373-522) ----
struct Song {
    std::string path;
    std::optional<std::string> artist, title, album, album_artist, genre;
    std::optional<int32_t> track_number, disc_number;
    double duration = 0.0;
    Analysis analysis;
    FeaturesVersion features_version = LATEST;

    static Analysis analyze(const std::vector<float>& sample_array) { return analyze_with_options(sample_array, AnalysisOptions{}); }
    // One song through blissgpu_analyze: safe from any number of threads (the reference's worker pool,
    // src/song/decoder.rs:299-329); concurrent calls are coalesced into one device batch inside the library.
    static Analysis analyze_with_options(const std::vector<float>& sample_array, const AnalysisOptions& opt) {
        std::vector<float> out(feature_count(opt.features_version));
        int32_t status = 0;
        const float dummy = 0.0f;
        check(blissgpu_analyze(sample_array.empty() ? &dummy : sample_array.data(), sample_array.size(),
                               static_cast<uint32_t>(opt.features_version), out.data(), &status));
        if (status != BLISSGPU_SONG_OK) throw AnalysisError("empty or too short song.");  // Err(...), src/song/mod.rs:426-430
        return Analysis(std::move(out), opt.features_version);
    }
    // Raw decoder output: `channels` interleaved channels of f32 (or s16, overload below) at 22 050 Hz; the mono downmix
    // ((L + R) * SQRT_2 / 2 for stereo, src/song/decoder/symphonia.rs:266-300) runs on the device.
    static Analysis analyze_interleaved(const std::vector<float>& samples, uint32_t channels, const AnalysisOptions& opt = {}) {
        return analyze_raw(samples.data(), BLISSGPU_SAMPLE_F32, channels, samples.size() / (channels ? channels : 1), opt);
    }
    static Analysis analyze_interleaved(const std::vector<int16_t>& samples, uint32_t channels, const AnalysisOptions& opt = {}) {
        return analyze_raw(samples.data(), BLISSGPU_SAMPLE_S16, channels, samples.size() / (channels ? channels : 1), opt);
    }
    static Analysis analyze_raw(const void* pcm, int sample_format, uint32_t channels, uint64_t frames, const AnalysisOptions& opt) {
        std::vector<float> out(feature_count(opt.features_version));
        int32_t status = 0;
        const float dummy = 0.0f;
        check(blissgpu_analyze_interleaved(frames ? pcm : &dummy, sample_format, channels, frames,
                                           static_cast<uint32_t>(opt.features_version), out.data(), &status));
        if (status != BLISSGPU_SONG_OK) throw AnalysisError("empty or too short song.");
        return Analysis(std::move(out), opt.features_version);
    }
    // Decoder output at ANY sample rate (`channels` interleaved channels of f32 / s16 / s32): what FFmpegDecoder::decode does
    // before Song::analyze -- libswresample to mono 22 050 Hz, src/song/decoder/ffmpeg.rs:36-109 -- runs on the device,
    // bit for bit (pinned by the reference's Adler-32 decoder tests, ffmpeg.rs:433-452).
    static Analysis analyze_decoded(const std::vector<float>& samples, uint32_t channels, uint32_t sample_rate, const AnalysisOptions& opt = {}) {
        return analyze_decoded_raw(samples.data(), BLISSGPU_SAMPLE_F32, channels, samples.size() / (channels ? channels : 1), sample_rate, opt);
    }
    static Analysis analyze_decoded(const std::vector<int16_t>& samples, uint32_t channels, uint32_t sample_rate, const AnalysisOptions& opt = {}) {
        return analyze_decoded_raw(samples.data(), BLISSGPU_SAMPLE_S16, channels, samples.size() / (channels ? channels : 1), sample_rate, opt);
    }
    static Analysis analyze_decoded(const std::vector<int32_t>& samples, uint32_t channels, uint32_t sample_rate, const AnalysisOptions& opt = {}) {
        return analyze_decoded_raw(samples.data(), BLISSGPU_SAMPLE_S32, channels, samples.size() / (channels ? channels : 1), sample_rate, opt);
    }
    static Analysis analyze_decoded_raw(const void* pcm, int sample_format, uint32_t channels, uint64_t frames, uint32_t sample_rate,
                                        const AnalysisOptions& opt) {
        std::vector<float> out(feature_count(opt.features_version));
        int32_t status = 0;
        const float dummy = 0.0f;
        check(blissgpu_analyze_decoded(frames ? pcm : &dummy, sample_format, channels, frames, sample_rate,
                                       static_cast<uint32_t>(opt.features_version), out.data(), &status));
        if (status != BLISSGPU_SONG_OK) throw AnalysisError("empty or too short song.");
        return Analysis(std::move(out), opt.features_version);
    }
    float distance(const Song& other) const { return analysis.distance(other.analysis); }
};

// Bulk form for a library as it comes off the decoders: every song with its own buffer, format, channel count and rate
// (blissgpu_analyze_batch_decoded); the compute half of analyze_paths_with_options (src/song/decoder.rs:278-332) for a host
// that keeps its decoder and drops the resampler.
inline std::vector<BlissResult<Analysis>> analyze_decoded_batch(const std::vector<blissgpu_decoded_song>& songs, const AnalysisOptions& opt = {}) {
    const uint32_t n = static_cast<uint32_t>(songs.size());
    const size_t d = feature_count(opt.features_version);
    std::vector<float> out(n * d);
    std::vector<int32_t> status(n);
    if (n) check(blissgpu_analyze_batch_decoded(songs.data(), n, static_cast<uint32_t>(opt.features_version), out.data(), status.data()));
    std::vector<BlissResult<Analysis>> res;
    res.reserve(n);
    for (uint32_t i = 0; i < n; i++) {
        if (status[i] == BLISSGPU_SONG_OK) res.emplace_back(Analysis(std::vector<float>(out.begin() + i * d, out.begin() + (i + 1) * d), opt.features_version));
        else res.emplace_back(AnalysisError("empty or too short song."));
    }
    return res;
}

// ---- CUE tracks as slices of one decoded buffer: BlissCueFile::get_songs (src/cue.rs:205-246) ----
// An INDEX time as the `std::time::Duration` the sheet parser (rcue in the reference) hands to BlissCueFile.
struct CueIndex {
    uint64_t secs;
    uint32_t nanos;
    // `Duration::as_secs_f32`: (secs as f32) + (nanos as f32) / 1e9_f32 -- NOT the exact sum rounded once: the two differ in the
    // last bit for 72 of the 360 000 mm:ss:ff values of an 80-minute disc, and the sample index derived from it moves by one
    float as_secs_f32() const {
        const volatile float q = static_cast<float>(nanos) / 1e9f;  // (rounded before the add, whatever the contraction mode)
        return static_cast<float>(secs) + q;
    }
    // mm:ss:ff of the sheet (75 frames per second), integer nanoseconds truncated
    static CueIndex from_msf(uint64_t mm, uint64_t ss, uint64_t ff) { return {mm * 60 + ss, static_cast<uint32_t>(ff * 1000000000ull / 75)}; }
};
// (start, end) sample ranges of the tracks of one FILE entry: `(index.as_secs_f32() * SAMPLE_RATE as f32) as usize` for each
// track's first INDEX (src/cue.rs:214-215,232); the last track runs to the end of the decoded file.  index_seconds must hold
// `Duration::as_secs_f32()` values (a float computed as mm * 60 + ss + ff / 75 is not the same number): use the CueIndex form
inline std::vector<std::pair<uint64_t, uint64_t>> cue_track_bounds(const std::vector<float>& index_seconds, uint64_t n_samples) {
    std::vector<std::pair<uint64_t, uint64_t>> b;
    for (size_t i = 0; i < index_seconds.size(); i++) {
        const uint64_t s = (uint64_t)(index_seconds[i] * (float)BLISSGPU_SAMPLE_RATE);
        const uint64_t e = i + 1 < index_seconds.size() ? (uint64_t)(index_seconds[i + 1] * (float)BLISSGPU_SAMPLE_RATE) : n_samples;
        b.emplace_back(s, e);
    }
    return b;
}
inline std::vector<std::pair<uint64_t, uint64_t>> cue_track_bounds(const std::vector<CueIndex>& index, uint64_t n_samples) {
    std::vector<float> secs;
    for (const CueIndex& ix : index) secs.push_back(ix.as_secs_f32());
    return cue_track_bounds(secs, n_samples);
}
// The audio file of a CUE sheet as the decoder delivered it (`frames` frames of `channels` interleaved samples at `sample_rate`) ->
// one result per track: the file is converted ONCE to mono 22 050 Hz on the device (FFmpegDecoder's conversion), the tracks are
// (offset, length) slices of that device buffer.  Sheet parsing (the reference uses the rcue crate) stays with the host.
// ctx: the context to run on; NULL = the library's first default context (borrowed: the one the entry points without a context
// argument use -- no context is created or destroyed per CUE file).
inline std::vector<BlissResult<Analysis>> analyze_cue_tracks(const void* pcm, int sample_format, uint32_t channels, uint64_t frames,
                                                             uint32_t sample_rate, const std::vector<float>& index_seconds,
                                                             const AnalysisOptions& opt = {}, blissgpu_ctx* ctx = nullptr) {
    struct Dev {  // device scratch of this call
        blissgpu_ctx* ctx = nullptr;
        void *raw = nullptr, *mono = nullptr, *rows = nullptr, *status = nullptr;
        ~Dev() { blissgpu_free(raw); blissgpu_free(mono); blissgpu_free(rows); blissgpu_free(status); }
    } d;
    if (channels == 0 || channels > 8) throw DecodingError("channels must be 1..8");
    if (sample_format != BLISSGPU_SAMPLE_F32 && sample_format != BLISSGPU_SAMPLE_S16 && sample_format != BLISSGPU_SAMPLE_S32)
        throw DecodingError("sample_format must be F32, S16 or S32");
    d.ctx = ctx;
    if (!d.ctx) check(blissgpu_default_ctx(0, &d.ctx));
    const size_t sample_bytes = sample_format == BLISSGPU_SAMPLE_S16 ? 2 : 4;
    const uint64_t n_mono = blissgpu_resampled_len(frames, sample_rate);
    const auto bounds = cue_track_bounds(index_seconds, n_mono);
    const uint32_t n = static_cast<uint32_t>(bounds.size());
    const size_t dft = feature_count(opt.features_version);
    std::vector<uint64_t> off(n), len(n);
    for (uint32_t i = 0; i < n; i++) {
        if (bounds[i].first > bounds[i].second || bounds[i].second > n_mono) throw DecodingError("CUE index beyond the end of the audio file");
        off[i] = bounds[i].first;
        len[i] = bounds[i].second - bounds[i].first;
    }
    check(blissgpu_malloc(&d.raw, std::max<uint64_t>(1, frames * channels * sample_bytes)));
    check(blissgpu_malloc(&d.mono, std::max<uint64_t>(1, n_mono) * 4 + 256));
    check(blissgpu_malloc(&d.rows, std::max<size_t>(1, n * dft) * 4));
    check(blissgpu_malloc(&d.status, std::max<uint32_t>(1, n) * 4));
    if (frames) check(blissgpu_memcpy_h2d(d.ctx, d.raw, pcm, frames * channels * sample_bytes));
    check(blissgpu_pcm_decode_device(d.ctx, d.raw, sample_format, channels, frames, sample_rate, static_cast<float*>(d.mono)));
    std::vector<float> out(n * dft);
    std::vector<int32_t> status(n);
    if (n) {
        check(blissgpu_analyze_batch_device(d.ctx, static_cast<const float*>(d.mono), off.data(), len.data(), n,
                                            static_cast<uint32_t>(opt.features_version), static_cast<float*>(d.rows),
                                            static_cast<int32_t*>(d.status)));
        check(blissgpu_memcpy_d2h(d.ctx, out.data(), d.rows, out.size() * 4));
        check(blissgpu_memcpy_d2h(d.ctx, status.data(), d.status, status.size() * 4));
    }
    std::vector<BlissResult<Analysis>> res;
    res.reserve(n);
    for (uint32_t i = 0; i < n; i++) {
        if (status[i] == BLISSGPU_SONG_OK) res.emplace_back(Analysis(std::vector<float>(out.begin() + i * dft, out.begin() + (i + 1) * dft), opt.features_version));
        else res.emplace_back(AnalysisError("empty or too short song."));
    }
    return res;
}
inline std::vector<BlissResult<Analysis>> analyze_cue_tracks(const void* pcm, int sample_format, uint32_t channels, uint64_t frames,
                                                             uint32_t sample_rate, const std::vector<CueIndex>& index,
                                                             const AnalysisOptions& opt = {}, blissgpu_ctx* ctx = nullptr) {
    std::vector<float> secs;
    for (const CueIndex& ix : index) secs.push_back(ix.as_secs_f32());
    return analyze_cue_tracks(pcm, sample_format, channels, frames, sample_rate, secs, opt, ctx);
}

// ---- Decoder trait (src/song/decoder.rs:34-333) ----
struct PreAnalyzedSong {
    std::string path;
    std::optional<std::string> artist, title, album, album_artist, genre;
    std::optional<int32_t> track_number, disc_number;
    double duration = 0.0;
    std::vector<float> sample_array;
    Song to_song(Analysis a, FeaturesVersion v) const {
        Song s;
        s.path = path; s.artist = artist; s.title = title; s.album = album; s.album_artist = album_artist; s.genre = genre;
        s.track_number = track_number; s.disc_number = disc_number; s.duration = duration;
        s.analysis = std::move(a); s.features_version = v;
        return s;
    }
};

class Decoder {
  public:
    virtual ~Decoder() = default;
    // required method (src/song/decoder.rs:129): file -> mono 22 050 Hz f32 samples; throws BlissError
    virtual PreAnalyzedSong decode(const std::string& path) const = 0;

    Song song_from_path(const std::string& path) const { return song_from_path_with_options(path, AnalysisOptions{}); }
    Song song_from_path_with_options(const std::string& path, const AnalysisOptions& opt) const {
        PreAnalyzedSong pre = decode(path);
        return pre.to_song(Song::analyze_with_options(pre.sample_array, opt), opt.features_version);
    }
    // (path, Result) pairs; a bad file never aborts the run (src/song/decoder.rs:313-325)
    std::vector<std::pair<std::string, BlissResult<Song>>> analyze_paths(const std::vector<std::string>& paths, const AnalysisOptions& opt = {}) const {
        std::vector<std::pair<std::string, BlissResult<Song>>> out;
        std::vector<PreAnalyzedSong> pending;
        for (const auto& p : paths) {
            try { pending.push_back(decode(p)); }
            catch (const BlissError& e) { out.emplace_back(p, e); }
        }
        std::vector<std::vector<float>> pcm;
        pcm.reserve(pending.size());
        for (auto& s : pending) pcm.push_back(s.sample_array);
        auto res = analyze_batch(pcm, opt);
        for (size_t i = 0; i < pending.size(); i++) {
            if (auto* e = std::get_if<BlissError>(&res[i])) out.emplace_back(pending[i].path, *e);
            else out.emplace_back(pending[i].path, pending[i].to_song(std::get<Analysis>(std::move(res[i])), opt.features_version));
        }
        return out;
    }
};

// ---- FLAC: the file goes to the device compressed; the host reads STREAMINFO and the VORBIS_COMMENT block only ----
struct FlacFile {
    PreAnalyzedSong pre;          // tags and duration; sample_array stays empty
    std::vector<uint8_t> bytes;   // the compressed file
};

// what to check beyond the structure (every frame stops 2 bytes before the next), on the device
enum class FlacVerify : uint32_t { None = 0, Crc = BLISSGPU_FLAC_CHECK_CRC16, Md5 = BLISSGPU_FLAC_CHECK_CRC16 | BLISSGPU_FLAC_CHECK_MD5 };

struct FlacVerdict {              // what the device found in one file (FlacDecoder::verify_paths)
    uint32_t flags = 0;           // BLISSGPU_FLAC_BAD_STREAM | _BAD_CRC16 | _BAD_MD5 | _MD5_UNCHECKED
    std::optional<uint32_t> first_bad_frame;  // the first frame whose CRC-16 failed
    std::optional<std::array<uint8_t, 16>> md5;  // the digest of the decoded audio, when it was computed
    bool ok() const { return (flags & 7u) == 0; }
    bool stream_ok() const { return !(flags & BLISSGPU_FLAC_BAD_STREAM); }
    bool crc_ok() const { return stream_ok() && !(flags & BLISSGPU_FLAC_BAD_CRC16); }
    const char* md5_state() const { return (flags & BLISSGPU_FLAC_BAD_MD5) ? "mismatch" : (flags & BLISSGPU_FLAC_MD5_UNCHECKED) ? "unchecked" : "match"; }
};

class FlacDecoder {
  public:
    // file -> tags + the compressed bytes (artist, title, album, album_artist, track_number, disc_number, genre as the
    // reference's FFmpeg decoder fills them, src/song/decoder/ffmpeg.rs:200-247; the duration from STREAMINFO); throws BlissError
    static FlacFile decode(const std::string& path) {
        FlacFile f;
        f.pre.path = path;
        FILE* fp = fopen(path.c_str(), "rb");
        if (!fp) throw DecodingError("while opening format for file '" + path + "'");
        uint8_t buf[65536];
        for (size_t k; (k = fread(buf, 1, sizeof(buf), fp)) > 0;) f.bytes.insert(f.bytes.end(), buf, buf + k);
        fclose(fp);
        const std::vector<uint8_t>& d = f.bytes;
        size_t p = 0;
        if (d.size() >= 10 && d[0] == 'I' && d[1] == 'D' && d[2] == '3')
            p = 10 + (size_t(d[6] & 0x7F) << 21 | size_t(d[7] & 0x7F) << 14 | size_t(d[8] & 0x7F) << 7 | size_t(d[9] & 0x7F)) + ((d[5] & 0x10) ? 10 : 0);
        if (p + 4 > d.size() || std::string(d.begin() + p, d.begin() + p + 4) != "fLaC") throw DecodingError("'" + path + "' is not a FLAC stream");
        p += 4;
        uint64_t rate = 0, total = 0;
        for (;;) {
            if (p + 4 > d.size()) throw DecodingError("'" + path + "' is truncated in the metadata");
            const uint8_t kind = d[p];
            const size_t len = size_t(d[p + 1]) << 16 | size_t(d[p + 2]) << 8 | d[p + 3];
            p += 4;
            if (len > d.size() - p) throw DecodingError("'" + path + "' is truncated in the metadata");
            if ((kind & 0x7F) == 0 && len >= 18) {
                uint64_t v = 0;
                for (size_t i = 10; i < 18; i++) v = (v << 8) | d[p + i];
                rate = v >> 44;
                total = v & ((1ull << 36) - 1);
            } else if ((kind & 0x7F) == 4) {
                comments(d.data() + p, len, &f.pre);
            }
            p += len;
            if (kind & 0x80) break;
        }
        if (!rate) throw DecodingError("'" + path + "' has no STREAMINFO");
        f.pre.duration = double(total) / double(rate);
        return f;
    }

    // `flac -t` for a batch of files, on the device: every frame's CRC-16 and (md5) the MD5 of the decoded audio against
    // STREAMINFO's -- one lane per song, slow for long songs; no analysis.  An unreadable file is BAD_STREAM
    static std::vector<std::pair<std::string, FlacVerdict>> verify_paths(const std::vector<std::string>& paths, bool md5 = true) {
        const size_t n = paths.size();
        std::vector<std::vector<uint8_t>> bytes(n);
        std::vector<const void*> files(n);
        std::vector<uint64_t> sizes(n);
        for (size_t i = 0; i < n; i++) {
            if (FILE* fp = fopen(paths[i].c_str(), "rb")) {
                uint8_t buf[65536];
                for (size_t k; (k = fread(buf, 1, sizeof(buf), fp)) > 0;) bytes[i].insert(bytes[i].end(), buf, buf + k);
                fclose(fp);
            }
            files[i] = bytes[i].data();
            sizes[i] = bytes[i].size();
        }
        std::vector<uint32_t> flags(n, 0), first_bad(n, 0xFFFFFFFFu);
        std::vector<uint8_t> digests(16 * n, 0);
        const uint32_t checks = BLISSGPU_FLAC_CHECK_CRC16 | (md5 ? BLISSGPU_FLAC_CHECK_MD5 : 0u);
        if (n) check(blissgpu_flac_verify_batch(files.data(), sizes.data(), static_cast<uint32_t>(n), checks, flags.data(), first_bad.data(), digests.data()));
        std::vector<std::pair<std::string, FlacVerdict>> out;
        for (size_t i = 0; i < n; i++) {
            FlacVerdict v;
            v.flags = flags[i];
            if (first_bad[i] != 0xFFFFFFFFu) v.first_bad_frame = first_bad[i];
            if (!(flags[i] & (BLISSGPU_FLAC_MD5_UNCHECKED | BLISSGPU_FLAC_BAD_STREAM))) {
                std::array<uint8_t, 16> d;
                std::copy(digests.begin() + 16 * i, digests.begin() + 16 * (i + 1), d.begin());
                v.md5 = d;
            }
            out.emplace_back(paths[i], v);
        }
        return out;
    }

    // (path, Result) pairs from ONE device batch of compressed files; a bad file yields its DecodingError and never aborts the run.
    // verify: also check every frame's CRC-16 (and the stream's MD5) on the device; a song that fails yields a DecodingError
    // that names the check and the frame
    static std::vector<std::pair<std::string, BlissResult<Song>>> analyze_paths(const std::vector<std::string>& paths, const AnalysisOptions& opt = {},
                                                                               FlacVerify verify = FlacVerify::None) {
        std::vector<std::pair<std::string, BlissResult<Song>>> out;
        std::vector<FlacFile> pending;
        for (const auto& p : paths) {
            try { pending.push_back(decode(p)); }
            catch (const BlissError& e) { out.emplace_back(p, e); }
        }
        const uint32_t d = blissgpu_feature_count(static_cast<uint32_t>(opt.features_version));
        const size_t n = pending.size();
        std::vector<const void*> files(n);
        std::vector<uint64_t> sizes(n);
        for (size_t i = 0; i < n; i++) { files[i] = pending[i].bytes.data(); sizes[i] = pending[i].bytes.size(); }
        std::vector<float> rows(n * d);
        std::vector<int32_t> status(n, 0);
        std::vector<uint32_t> flags(n, BLISSGPU_FLAC_BAD_STREAM), first_bad(n, 0xFFFFFFFFu);
        if (n && verify == FlacVerify::None)
            check(blissgpu_analyze_batch_flac(files.data(), sizes.data(), static_cast<uint32_t>(n), static_cast<uint32_t>(opt.features_version), rows.data(), status.data()));
        else if (n)
            check(blissgpu_analyze_batch_flac_verified(files.data(), sizes.data(), static_cast<uint32_t>(n), static_cast<uint32_t>(opt.features_version),
                                                       static_cast<uint32_t>(verify), rows.data(), status.data(), flags.data(), first_bad.data()));
        for (size_t i = 0; i < n; i++) {
            if (status[i] == BLISSGPU_SONG_OK)
                out.emplace_back(pending[i].pre.path, pending[i].pre.to_song(Analysis(std::vector<float>(rows.begin() + i * d, rows.begin() + (i + 1) * d), opt.features_version), opt.features_version));
            else if (status[i] == BLISSGPU_SONG_TOO_SHORT) out.emplace_back(pending[i].pre.path, AnalysisError("empty or too short song."));
            else if (flags[i] & BLISSGPU_FLAC_BAD_STREAM) out.emplace_back(pending[i].pre.path, DecodingError("the FLAC stream of '" + pending[i].pre.path + "' cannot be decoded"));
            else if (flags[i] & BLISSGPU_FLAC_BAD_CRC16)
                out.emplace_back(pending[i].pre.path, DecodingError("the FLAC stream of '" + pending[i].pre.path + "' is damaged: CRC-16 mismatch in frame " + std::to_string(first_bad[i])));
            else out.emplace_back(pending[i].pre.path, DecodingError("the FLAC stream of '" + pending[i].pre.path + "' is damaged: the MD5 of the decoded audio is not STREAMINFO's"));
        }
        return out;
    }

  private:
    static std::optional<int32_t> number(const std::string& t) {  // "2" or "02/05" (ffmpeg.rs:224-241)
        auto parse = [](const std::string& x) -> std::optional<int32_t> {
            if (x.empty()) return std::nullopt;
            size_t i = (x[0] == '-' || x[0] == '+') ? 1 : 0;
            if (i == x.size() || x.size() - i > 10) return std::nullopt;
            int64_t v = 0;
            for (; i < x.size(); i++) {
                if (x[i] < '0' || x[i] > '9') return std::nullopt;
                v = v * 10 + (x[i] - '0');
            }
            if (x[0] == '-') v = -v;
            if (v < INT32_MIN || v > INT32_MAX) return std::nullopt;
            return static_cast<int32_t>(v);
        };
        if (auto v = parse(t)) return v;
        const size_t slash = t.find('/');
        return slash == std::string::npos ? std::nullopt : parse(t.substr(0, slash));
    }
    static void comments(const uint8_t* b, size_t n, PreAnalyzedSong* s) {
        auto u32 = [&](size_t p) { return size_t(b[p]) | size_t(b[p + 1]) << 8 | size_t(b[p + 2]) << 16 | size_t(b[p + 3]) << 24; };
        if (n < 8) return;
        size_t p = 4 + u32(0);
        if (p + 4 > n) return;
        const size_t count = u32(p);
        p += 4;
        std::map<std::string, std::string> tags;
        for (size_t i = 0; i < count && p + 4 <= n; i++) {
            const size_t len = u32(p);
            p += 4;
            if (len > n - p) return;
            const std::string entry(reinterpret_cast<const char*>(b + p), len);
            p += len;
            const size_t eq = entry.find('=');
            if (eq == std::string::npos) continue;
            std::string key = entry.substr(0, eq);
            for (char& ch : key) ch = static_cast<char>(std::tolower(static_cast<unsigned char>(ch)));
            if (key == "tracknumber") key = "track";
            else if (key == "discnumber") key = "disc";
            else if (key == "albumartist") key = "album_artist";
            auto it = tags.find(key);
            if (it == tags.end()) tags[key] = entry.substr(eq + 1);
            else it->second += ";" + entry.substr(eq + 1);
        }
        auto text = [&](const char* k) -> std::optional<std::string> {
            auto it = tags.find(k);
            return it == tags.end() || it->second.empty() ? std::nullopt : std::optional<std::string>(it->second);
        };
        s->artist = text("artist"); s->title = text("title"); s->album = text("album"); s->album_artist = text("album_artist");
        s->genre = text("genre");
        if (auto t = text("track")) s->track_number = number(*t);
        if (auto t = text("disc")) s->disc_number = number(*t);
    }
};

// ---- playlist ordering (src/playlist.rs:24-59, 173-221, 256-402); distances are evaluated on the GPU ----
// A metric builder names one of the device metrics (the reference's `&dyn DistanceMetricBuilder` implemented by the
// plain distance functions, src/playlist.rs:41-59); the metric it builds from a set of vectors is the sum of the
// distances to each vector of the set.
struct MetricBuilder {
    int metric = BLISSGPU_METRIC_EUCLIDEAN;
    std::vector<float> m;  // d x d row-major for MAHALANOBIS
    const float* mptr() const { return m.empty() ? nullptr : m.data(); }
};
inline MetricBuilder euclidean_builder() { return {BLISSGPU_METRIC_EUCLIDEAN, {}}; }
inline MetricBuilder cosine_builder() { return {BLISSGPU_METRIC_COSINE, {}}; }
inline MetricBuilder mahalanobis_builder(std::vector<float> m) { return {BLISSGPU_METRIC_MAHALANOBIS, std::move(m)}; }

inline void check_ordering(int rc) {  // n32() / argmin().unwrap() panic on NaN in the reference
    if (rc == BLISSGPU_ERR_NAN) throw std::domain_error("NaN distance");
    check(rc);
}

template <typename T>
const Song& as_song(const T& s) { return s; }          // AsRef<Song>: specialise for wrapper types
template <typename T>
const Song& as_song(T* const& s) { return as_song(*s); }

template <typename T>
std::vector<float> feature_matrix(const std::vector<T>& songs, size_t& d) {
    std::vector<float> x;
    d = songs.empty() ? 0 : as_song(songs[0]).analysis.as_vec().size();
    for (const auto& s : songs) {
        const auto& v = as_song(s).analysis.as_vec();
        if (v.size() != d) throw std::logic_error("Mismatched features version between two songs or analysis");
        x.insert(x.end(), v.begin(), v.end());
    }
    return x;
}

// closest_to_songs (src/playlist.rs:256-270)
template <typename T>
std::vector<T> closest_to_songs(const std::vector<T>& initial_songs, const std::vector<T>& candidate_songs, const MetricBuilder& mb) {
    if (candidate_songs.empty()) return {};
    size_t d = 0, ds = 0;
    const auto x = feature_matrix(candidate_songs, d);
    const auto s = feature_matrix(initial_songs, ds);
    std::vector<uint32_t> order(candidate_songs.size());
    check_ordering(blissgpu_closest_to_songs(s.data(), (uint32_t)initial_songs.size(), x.data(), candidate_songs.size(), (uint32_t)d,
                                             mb.metric, mb.mptr(), order.data(), nullptr));
    std::vector<T> out;
    for (uint32_t i : order) out.push_back(candidate_songs[i]);
    return out;
}

// extended_isolation_forest::ForestOptions as a metric builder (src/playlist.rs:230-251) plus the seed that makes the
// forest -- and so the playlist -- reproducible.  max_tree_depth 0 = None (ceil(log2(min(sample_size, seeds)))).
struct ForestOptions {
    uint32_t n_trees;
    uint32_t sample_size;
    uint32_t max_tree_depth;
    uint32_t extension_level;
    uint64_t seed;
};

// closest_to_songs with the forest metric (src/playlist.rs:256-270): the forest is built on the host from the initial
// songs (at least two, or std::invalid_argument from check()), the candidates are scored and ordered on the GPU.
template <typename T>
std::vector<T> closest_to_songs(const std::vector<T>& initial_songs, const std::vector<T>& candidate_songs, const ForestOptions& opts) {
    if (candidate_songs.empty()) return {};
    size_t d = 0, ds = 0;
    const auto x = feature_matrix(candidate_songs, d);
    const auto s = feature_matrix(initial_songs, ds);
    if (!initial_songs.empty() && ds != d) throw std::logic_error("Mismatched features version between two songs or analysis");
    void* forest = nullptr;
    check(blissgpu_forest_build(s.data(), initial_songs.size(), (uint32_t)d, opts.n_trees, opts.sample_size, opts.max_tree_depth,
                                opts.extension_level, opts.seed, &forest));
    std::vector<uint32_t> order(candidate_songs.size());
    const int rc = blissgpu_forest_closest_to_songs(forest, x.data(), candidate_songs.size(), order.data(), nullptr);
    blissgpu_forest_destroy(forest);
    check(rc);
    std::vector<T> out;
    for (uint32_t i : order) out.push_back(candidate_songs[i]);
    return out;
}

// closest_to_songs with the forest metric for every GROUP of songs in one call, cut after k: one forest per group (same
// options, same seed), the group's own songs left out when exclude_members (the first candidate equal to each member).  A
// group with min(sample_size, members) < 2 has no forest and gets an empty list.
template <typename T>
std::vector<std::vector<T>> forest_group_playlists(const std::vector<std::vector<T>>& groups, const std::vector<T>& candidate_songs,
                                                   uint32_t k, const ForestOptions& opts, bool exclude_members = true) {
    std::vector<std::vector<T>> out(groups.size());
    if (groups.empty() || candidate_songs.empty()) return out;
    size_t d = 0, ds = 0;
    const auto x = feature_matrix(candidate_songs, d);
    std::vector<T> flat;
    std::vector<uint64_t> off(groups.size() + 1, 0);
    for (size_t g = 0; g < groups.size(); g++) {
        flat.insert(flat.end(), groups[g].begin(), groups[g].end());
        off[g + 1] = flat.size();
    }
    const auto s = feature_matrix(flat, ds);
    if (!flat.empty() && ds != d) throw std::logic_error("Mismatched features version between two songs or analysis");
    std::vector<uint32_t> skip(flat.size(), 0xFFFFFFFFu);
    if (exclude_members)
        for (size_t i = 0; i < flat.size(); i++)
            for (size_t j = 0; j < candidate_songs.size(); j++) {
                const Song &a = as_song(candidate_songs[j]), &b = as_song(flat[i]);
                if (a.path == b.path && a.analysis == b.analysis && a.album == b.album && a.title == b.title && a.artist == b.artist &&
                    a.track_number == b.track_number && a.disc_number == b.disc_number) { skip[i] = (uint32_t)j; break; }
            }
    std::vector<uint32_t> idx(groups.size() * (size_t)k);
    check(blissgpu_group_forest_knn(s.data(), off.data(), groups.size(), x.data(), candidate_songs.size(), (uint32_t)d, opts.n_trees,
                                    opts.sample_size, opts.max_tree_depth, opts.extension_level, opts.seed, skip.data(), k, idx.data(),
                                    nullptr, nullptr));
    for (size_t g = 0; g < groups.size(); g++)
        for (uint32_t i = 0; i < k; i++)
            if (idx[g * k + i] != 0xFFFFFFFFu) out[g].push_back(candidate_songs[idx[g * k + i]]);
    return out;
}

// closest_to_songs for many single seeds at once, cut after k (src/playlist.rs:256-270; Library::playlist_from(&[song])
// .take(k), src/library.rs:762-850): row i of idx = the k candidates closest to queries[i] in ascending distance, equal
// distances in candidate order, without candidate skip[i] (0xFFFFFFFF: none); short rows end in 0xFFFFFFFF / +inf.
// queries / candidates are row-major q x d / n x d; one device call, no distance matrix.
struct NearestOrder { std::vector<uint32_t> idx; std::vector<float> dist; };
inline NearestOrder nearest_order(const std::vector<float>& queries, size_t q, const std::vector<float>& candidates, size_t n, size_t d,
                                  uint32_t k, const MetricBuilder& mb, const std::vector<uint32_t>* skip = nullptr) {
    NearestOrder out{std::vector<uint32_t>(q * k), std::vector<float>(q * k)};
    check_ordering(blissgpu_knn(queries.data(), q, candidates.data(), n, (uint32_t)d, mb.metric, mb.mptr(), skip ? skip->data() : nullptr,
                                k, out.idx.data(), out.dist.data()));
    return out;
}

// for every song: closest_to_songs(&[song], candidate_songs, metric)[..k]; exclude_self leaves out the first candidate whose
// Song equals the query song (Song: PartialEq, compared as closest_album_to_group does)
template <typename T>
std::vector<std::vector<T>> nearest_songs(const std::vector<T>& songs, const std::vector<T>& candidate_songs, uint32_t k, const MetricBuilder& mb,
                                          bool exclude_self = false) {
    std::vector<std::vector<T>> out(songs.size());
    if (songs.empty() || candidate_songs.empty()) return out;
    size_t d = 0, dq = 0;
    const auto x = feature_matrix(candidate_songs, d);
    const auto s = feature_matrix(songs, dq);
    std::vector<uint32_t> skip(songs.size(), 0xFFFFFFFFu);
    if (exclude_self)
        for (size_t i = 0; i < songs.size(); i++)
            for (size_t j = 0; j < candidate_songs.size(); j++)
            {
                const Song &a = as_song(candidate_songs[j]), &b = as_song(songs[i]);
                if (a.path == b.path && a.analysis == b.analysis && a.album == b.album && a.title == b.title && a.artist == b.artist &&
                    a.track_number == b.track_number && a.disc_number == b.disc_number) { skip[i] = (uint32_t)j; break; }
            }
    const auto r = nearest_order(s, songs.size(), x, candidate_songs.size(), d, k, mb, &skip);
    for (size_t i = 0; i < songs.size(); i++)
        for (uint32_t c = 0; c < k; c++) {
            const uint32_t j = r.idx[i * k + c];
            if (j != 0xFFFFFFFFu) out[i].push_back(candidate_songs[j]);
        }
    return out;
}

// song_to_song (src/playlist.rs:272-326)
template <typename T>
std::vector<T> song_to_song(const std::vector<T>& initial_songs, const std::vector<T>& candidate_songs, const MetricBuilder& mb) {
    if (candidate_songs.empty()) return {};
    size_t d = 0, ds = 0;
    const auto x = feature_matrix(candidate_songs, d);
    const auto s = feature_matrix(initial_songs, ds);
    std::vector<uint32_t> order(candidate_songs.size());
    check_ordering(blissgpu_song_to_song(s.data(), (uint32_t)initial_songs.size(), x.data(), candidate_songs.size(), (uint32_t)d,
                                         mb.metric, mb.mptr(), order.data()));
    std::vector<T> out;
    for (uint32_t i : order) out.push_back(candidate_songs[i]);
    return out;
}

// dedup_playlist_custom_distance / dedup_playlist (src/playlist.rs:343-402)
template <typename T>
std::vector<T> dedup_playlist_custom_distance(const std::vector<T>& playlist, std::optional<float> distance_threshold, const MetricBuilder& mb) {
    if (playlist.empty()) return {};
    size_t d = 0;
    const auto x = feature_matrix(playlist, d);
    // one key per song for the title / artist rule: 0 when either is None, equal keys for equal (title, artist)
    std::map<std::pair<std::string, std::string>, uint32_t> seen;
    std::vector<uint32_t> meta(playlist.size(), 0);
    for (size_t i = 0; i < playlist.size(); i++) {
        const Song& s = as_song(playlist[i]);
        if (s.title && s.artist) meta[i] = seen.emplace(std::make_pair(*s.title, *s.artist), (uint32_t)seen.size() + 1).first->second;
    }
    std::vector<uint32_t> kept(playlist.size());
    uint64_t n_kept = 0;
    check_ordering(blissgpu_dedup_playlist(x.data(), playlist.size(), (uint32_t)d, nullptr, playlist.size(), meta.data(), mb.metric,
                                           mb.mptr(), distance_threshold.value_or(0.05f), kept.data(), &n_kept));
    std::vector<T> out;
    for (uint64_t k = 0; k < n_kept; k++) out.push_back(playlist[kept[k]]);
    return out;
}
template <typename T>
std::vector<T> dedup_playlist(const std::vector<T>& playlist, std::optional<float> distance_threshold) {
    return dedup_playlist_custom_distance(playlist, distance_threshold, euclidean_builder());
}

// duplicate_groups: the duplicate rule of dedup_playlist_custom_distance (src/playlist.rs:381-388) over EVERY pair of a
// collection, closed transitively -- the groups of two or more songs that are "the same song", ordered by their first member,
// members in the caller's order.  One device call, no distance matrix.
template <typename T>
std::vector<std::vector<T>> duplicate_groups(const std::vector<T>& songs, std::optional<float> distance_threshold, const MetricBuilder& mb) {
    if (songs.empty()) return {};
    size_t d = 0;
    const auto x = feature_matrix(songs, d);
    std::map<std::pair<std::string, std::string>, uint32_t> seen;
    std::vector<uint32_t> meta(songs.size(), 0);
    for (size_t i = 0; i < songs.size(); i++) {
        const Song& s = as_song(songs[i]);
        if (s.title && s.artist) meta[i] = seen.emplace(std::make_pair(*s.title, *s.artist), (uint32_t)seen.size() + 1).first->second;
    }
    std::vector<uint32_t> label(songs.size());
    uint64_t n_pairs = 0;
    check_ordering(blissgpu_duplicate_groups(x.data(), songs.size(), (uint32_t)d, meta.data(), mb.metric, mb.mptr(),
                                             distance_threshold.value_or(0.05f), label.data(), &n_pairs, nullptr, nullptr, 0));
    // a label is the smallest member: rows in order, so groups come by first member and members ascend
    std::map<uint32_t, std::vector<T>> by_label;
    for (size_t i = 0; i < songs.size(); i++) by_label[label[i]].push_back(songs[i]);
    std::vector<std::vector<T>> out;
    for (auto& kv : by_label)
        if (kv.second.size() >= 2) out.push_back(std::move(kv.second));
    return out;
}
template <typename T>
std::vector<std::vector<T>> duplicate_groups(const std::vector<T>& songs, std::optional<float> distance_threshold) {
    return duplicate_groups(songs, distance_threshold, euclidean_builder());
}

// closest_album_to_group (src/playlist.rs:424-485): the albums of `pool` (songs of `group` removed, songs without an
// album dropped) ordered by the euclidean distance of their mean analysis to the group's mean analysis, each album
// ordered by (disc number, track number); `group` itself comes first.
template <typename T>
std::vector<T> closest_album_to_group(const std::vector<T>& group, const std::vector<T>& pool_in) {
    if (group.empty()) throw ProviderError("Mean of empty slice");
    std::vector<T> pool;
    for (const auto& s : pool_in) {
        bool in_group = false;
        for (const auto& g : group) {
            const Song &a = as_song(g), &b = as_song(s);
            if (a.path == b.path && a.analysis == b.analysis && a.album == b.album && a.title == b.title && a.artist == b.artist &&
                a.track_number == b.track_number && a.disc_number == b.disc_number) { in_group = true; break; }
        }
        if (!in_group) pool.push_back(s);
    }
    const size_t d = as_song(group[0]).analysis.as_vec().size();
    auto mean_of = [&](const std::vector<const Song*>& songs) {  // ndarray mean_axis: sequential f32 row sum / n
        std::vector<float> m(d, 0.0f);
        for (const Song* s : songs) for (size_t k = 0; k < d; k++) m[k] = m[k] + s->analysis.as_vec()[k];
        for (size_t k = 0; k < d; k++) m[k] = m[k] / (float)songs.size();
        return m;
    };
    std::vector<std::string> names;
    std::vector<std::vector<const Song*>> members;
    for (const auto& s : pool) {
        const Song& song = as_song(s);
        if (!song.album) continue;
        size_t a = 0;
        while (a < names.size() && names[a] != *song.album) a++;
        if (a == names.size()) { names.push_back(*song.album); members.emplace_back(); }
        members[a].push_back(&song);
    }
    std::vector<const Song*> gs;
    for (const auto& g : group) gs.push_back(&as_song(g));
    const std::vector<float> first = mean_of(gs);
    std::vector<T> playlist = group;
    if (!names.empty()) {
        std::vector<float> means;
        for (const auto& m : members) { const auto v = mean_of(m); means.insert(means.end(), v.begin(), v.end()); }
        std::vector<uint32_t> order(names.size());
        check_ordering(blissgpu_closest_to_songs(first.data(), 1, means.data(), names.size(), (uint32_t)d, BLISSGPU_METRIC_EUCLIDEAN,
                                                 nullptr, order.data(), nullptr));
        for (uint32_t a : order) {
            std::vector<T> al;
            for (const auto& s : pool) if (as_song(s).album && *as_song(s).album == names[a]) al.push_back(s);
            std::stable_sort(al.begin(), al.end(), [](const T& x, const T& y) {  // Option<i32>: None < Some
                const Song &p = as_song(x), &q = as_song(y);
                return std::make_pair(p.disc_number, p.track_number) < std::make_pair(q.disc_number, q.track_number);
            });
            playlist.insert(playlist.end(), al.begin(), al.end());
        }
    }
    return playlist;
}

// variance_based_weight_matrix (src/playlist.rs:173-221): d x d row-major; host arithmetic in the reference's order
inline std::vector<float> variance_based_weight_matrix(const std::vector<std::vector<float>>& seeds) {
    if (seeds.size() < 2) throw ProviderError("seeds must contain more than one element");
    const size_t n = seeds[0].size();
    if (n == 0) throw ProviderError("seed feature vectors must not be empty");
    for (const auto& s : seeds) if (s.size() != n) throw ProviderError("all seed feature vectors must have the same length");
    const float ns = (float)seeds.size();
    std::vector<float> mean(n, 0.0f), var(n, 0.0f);
    for (const auto& s : seeds) for (size_t k = 0; k < n; k++) mean[k] = mean[k] + s[k];
    for (size_t k = 0; k < n; k++) mean[k] = mean[k] / ns;
    for (const auto& s : seeds) for (size_t k = 0; k < n; k++) { const float diff = s[k] - mean[k]; var[k] = var[k] + diff * diff; }
    for (size_t k = 0; k < n; k++) { var[k] = var[k] / ns; var[k] = 1.0f / (var[k] + 1e-6f); }
    float p[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sum = 0.0f;  // ndarray sum(): unrolled_fold
    size_t k = 0;
    for (; k + 8 <= n; k += 8) for (int u = 0; u < 8; u++) p[u] = p[u] + var[k + u];
    sum = sum + (p[0] + p[4]); sum = sum + (p[1] + p[5]); sum = sum + (p[2] + p[6]); sum = sum + (p[3] + p[7]);
    for (; k < n; k++) sum = sum + var[k];
    const float scale = (float)n / sum;
    std::vector<float> m(n * n, 0.0f);
    for (size_t q = 0; q < n; q++) m[q * n + q] = var[q] * scale;
    return m;
}

}  // namespace bliss
