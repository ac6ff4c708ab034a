"""bliss_rs_amd -- MI355X-native implementation of bliss-rs's per-song analysis hot path
(`Song::analyze`) and feature-vector distances, behind the reference's own interface.

Host-side mirror of the reference surface (names, argument meaning and error behaviour follow
bliss-rs / `bliss-audio` 0.13.0):

    Song.analyze / Song.analyze_with_options      src/song/mod.rs:403-508
    Analysis, AnalysisIndex, FeaturesVersion      src/song/mod.rs:102-371, src/lib.rs:151-187
    Decoder.{decode, song_from_path, analyze_paths}  src/song/decoder.rs:115-333
    FlacDecoder, analyze_flac_batch, Context.flac_decode: .flac files decoded ON THE DEVICE, compressed bytes in, rows out
    flac_verify_batch, analyze_flac_batch(verify=), Context.flac_crc16 / flac_md5: frame CRC-16 and stream MD5 checked on the device
    cue.{cue_track_bounds, analyze_cue_tracks}    BlissCueFile::get_songs, src/cue.rs:205-246 (sheet parsing stays with the host)
    euclidean / cosine / mahalanobis distance, closest_to_songs, song_to_song, dedup, ...   src/playlist.rs
    playlist.nearest_order / nearest_songs, library.similar_songs: the k closest songs of many songs in one call
    playlist.nearest_to_groups / group_playlists, library.group_playlists: a k-song playlist per album / artist / seed set in one call
    playlist.nearest_albums / closest_albums_to_groups, library.album_playlists: every album followed by the albums most like it, one call
    playlist.duplicate_labels / duplicate_groups, library.duplicate_songs: the songs of a whole collection that are the same song
    playlist.group_neighbours, library.similar_groups / similar_artists / similar_artists_playlist: which artists (albums, genres) are like each other
    playlist.minimum_spanning_tree / core_distances, library.song_tree / linked_clusters / tour: clusters without k, the dendrogram, a tour of the library
    playlist.ward_tree / ward_nearest / choose_k_tree, library.ward_tree / ward_clusters: Ward's dendrogram -- compact clusters that nest, any k by cutting one tree
    playlist.kmedoids / pam_scan / medoid_songs, library.medoid_songs: k-medoids -- the k SONGS that summarise a library, under cosine too
    fingerprint_batch / fingerprint_decoded_batch, playlist.fingerprint_match / fingerprint_duplicates, library.fingerprint_duplicates: acoustic fingerprints -- the same RECORDING found again, whatever its features say
    loudness_batch / loudness_flac_batch / Loudness.replaygain, library.store_loudness / load_loudness / loudness_statistics: EBU R 128 loudness, range and true peak per song and album at the files' native rates -- ReplayGain without a second scanner
    playlist.local_scales / scaled_nearest_order / hubness, library.similar_songs_scaled / hubness / orphan_songs: lists that a few hub songs do not dominate, and a measure of how much they do
    playlist.ForestOptions / forest_scores: the extended isolation forest metric for several seed songs   src/playlist.rs:230-251
    library.{load_feature_matrix, load_songs, store_song}   feature table of src/library.rs:500-531, 1355-1372, 1560-1630
    library.{playlist_from, playlist_from_custom, album_playlist_from, songs_from_album}   src/library.rs:762-893

All compute goes through the C ABI of include/blissgpu.h (hand-written HIP kernels for gfx950);
there is no CPU fallback.
"""
from ._ffi import BlissGpuError, LIB_PATH  # noqa: F401
from .song import (  # noqa: F401
    SAMPLE_RATE, CHANNELS, NUMBER_FEATURES, Analysis, AnalysisError, AnalysisIndex, AnalysisIndexv1,
    AnalysisOptions, BlissError, DecodingError, FeaturesVersion, ProviderError, Song, analyze_batch, analyze_decoded_batch,
    FlacVerdict, analyze_flac_batch, flac_decode, flac_decode_batch, flac_verify_batch, resampled_len,
    FINGERPRINT_VERSION, fingerprint_batch, fingerprint_decoded_batch, fingerprint_len,
    LOUDNESS_VERSION, Loudness, loudness_batch, loudness_flac_batch, loudness_blocks, loudness_gate, loudness_range)
from .decoder import Decoder, FlacDecoder, PreAnalyzedSong, RawPcmDecoder  # noqa: F401
from . import playlist  # noqa: F401
from . import cue  # noqa: F401
from . import library  # noqa: F401
from .device import Context, Node  # noqa: F401

__version__ = "0.3.0"
