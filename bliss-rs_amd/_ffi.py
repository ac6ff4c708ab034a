"""ctypes binding of libblissgpu.so (the C ABI declared in include/blissgpu.h).

There is no CPU fallback: if the shared library is missing, or no HIP device is usable, every compute
call raises.  The library is loaded lazily so that `import bliss_rs_amd` (and the build check) works
on a machine without a GPU.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# BLISSGPU_LIB: developer aid for A/B timing of two builds of the library on the same box (never a CPU path)
LIB_PATH = os.environ.get("BLISSGPU_LIB") or os.path.join(_HERE, "libblissgpu.so")

OK, ERR_NO_DEVICE, ERR_INVALID, ERR_HIP, ERR_OOM, ERR_NAN, ERR_RCCL, ERR_TIMEOUT, ERR_INTERNAL = 0, 1, 2, 3, 4, 5, 6, 7, 8
SAMPLE_F32, SAMPLE_S16, SAMPLE_S32 = 0, 1, 2
SAMPLE_RATE = 22050
SONG_OK, SONG_TOO_SHORT, SONG_DECODE_ERROR = 0, 1, 2
FLAC_INFO_WORDS = 12
FLAC_CHECK_CRC16, FLAC_CHECK_MD5 = 1, 2
FLAC_BAD_STREAM, FLAC_BAD_CRC16, FLAC_BAD_MD5, FLAC_MD5_UNCHECKED = 1, 2, 4, 8
METRIC_EUCLIDEAN, METRIC_COSINE, METRIC_MAHALANOBIS = 0, 1, 2
CHAINS_AUTO, CHAINS_STEPS, CHAINS_LISTS = 0, 1, 2
JOURNEY_CHAIN, JOURNEY_WAYPOINT = 0, 1
GATE_NONE, GATE_UP, GATE_DOWN = 0, 1, 2
RADIO_CHAIN, RADIO_NEAREST, RADIO_MAX_RULES = 0, 1, 4
OPT_SERIAL, OPT_TAIL_MODE, OPT_PIPELINE_CHUNKS, OPT_CAND_BUDGET, OPT_ROLLOFF_EXACT_ALL, OPT_DEBUG_CHROMA, OPT_TAIL_SPLIT = 0, 1, 2, 3, 4, 5, 6
OPT_STFT_SHAPE = 7
OPT_FLUX_ORDER = 8
OPT_STAGE_LANES, OPT_STAGE_SLAB_KIB, OPT_STAGE_SLABS, OPT_STAGE_NUMA = 9, 10, 11, 12
OPT_FOREST_SPLIT, OPT_FOREST_WALK = 13, 14
OPT_FOREST_GROUP_NODES = 15
GROUP_OK, GROUP_TOO_FEW_SEEDS = 0, 1
KMEANS_MAX_K = 65535
METRIC_FORM_DIAGONAL, METRIC_FORM_FULL = 0, 1
LEARN_CONVERGED, LEARN_MAX_ITER, LEARN_DIVERGED = 0, 1, 2
COV_OK, COV_NOT_POSITIVE = 0, 1
MOMENTS_BLOCK = 256
GROUPS_SYMMETRIC, GROUPS_DIRECTED = 0, 1

# the names the Python API gives those constants (playlist.py binds them as _METRICS, _ROUTES, ...)
METRICS = {"euclidean": METRIC_EUCLIDEAN, "cosine": METRIC_COSINE, "mahalanobis": METRIC_MAHALANOBIS}
ROUTES = {"auto": CHAINS_AUTO, "steps": CHAINS_STEPS, "lists": CHAINS_LISTS}  # chain_order
JOURNEY_MODES = {"chain": JOURNEY_CHAIN, "waypoint": JOURNEY_WAYPOINT}  # journey_order
GATES = {None: GATE_NONE, "up": GATE_UP, "down": GATE_DOWN}
GROUP_MODES = {"symmetric": GROUPS_SYMMETRIC, "directed": GROUPS_DIRECTED}  # group_neighbours
RADIO_MODES = {"chain": RADIO_CHAIN, "nearest": RADIO_NEAREST}  # radio_order
FORMS = {"diagonal": METRIC_FORM_DIAGONAL, "full": METRIC_FORM_FULL}  # learn_metric

_f32p = C.POINTER(C.c_float)
_f64p = C.POINTER(C.c_double)
_u64p = C.POINTER(C.c_uint64)
_u32p = C.POINTER(C.c_uint32)
_i32p = C.POINTER(C.c_int32)
_vp = C.c_void_p



class DecodedSong(C.Structure):
    """blissgpu_decoded_song: one song as the decoder delivers it (host memory)."""
    _fields_ = [("pcm", C.c_void_p), ("frames", C.c_uint64), ("sample_rate", C.c_uint32), ("channels", C.c_uint16),
                ("sample_format", C.c_uint16)]


# name -> (restype, argtypes); must list every symbol include/blissgpu.h declares
SIGNATURES = {
    "blissgpu_analyze_decoded": (C.c_int, [_vp, C.c_int, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, _vp, _i32p]),
    "blissgpu_analyze_batch_decoded": (C.c_int, [C.POINTER(DecodedSong), C.c_uint32, C.c_uint32, _vp, _i32p]),
    "blissgpu_resampled_len": (C.c_uint64, [C.c_uint64, C.c_uint32]),
    "blissgpu_resample_filter": (C.c_int, [C.c_uint32, _vp, C.c_uint64, _u32p, _u32p]),
    "blissgpu_pcm_decode_device": (C.c_int, [_vp, _vp, C.c_int, C.c_uint32, C.c_uint64, C.c_uint32, _vp]),
    "blissgpu_flac_info": (C.c_int, [_vp, C.c_uint64, _u64p]),
    "blissgpu_flac_index": (C.c_int, [_vp, C.c_uint64, C.c_int, _u64p, _u64p, C.c_uint64, _u64p]),
    "blissgpu_flac_decode_device": (C.c_int, [_vp, _vp, C.c_uint64, _u64p, C.c_uint64, _u64p, _vp, _vp, _vp]),
    "blissgpu_flac_decode": (C.c_int, [_vp, C.c_uint64, _vp, C.c_uint64, _u64p, _i32p]),
    "blissgpu_flac_decode_batch": (C.c_int, [C.POINTER(_vp), _u64p, C.c_uint32, C.POINTER(_vp), _u64p, _u64p, _i32p]),
    "blissgpu_analyze_batch_flac": (C.c_int, [C.POINTER(_vp), _u64p, C.c_uint32, C.c_uint32, _vp, _i32p]),
    "blissgpu_ctx_flac_slow_songs": (C.c_uint64, [_vp]),
    "blissgpu_flac_verify_batch": (C.c_int, [C.POINTER(_vp), _u64p, C.c_uint32, C.c_uint32, _u32p, _u32p, _vp]),
    "blissgpu_analyze_batch_flac_verified": (C.c_int, [C.POINTER(_vp), _u64p, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _i32p, _u32p, _u32p]),
    "blissgpu_flac_crc16_device": (C.c_int, [_vp, _vp, C.c_uint64, _u64p, C.c_uint64, _vp, _vp, _vp]),
    "blissgpu_flac_md5_device": (C.c_int, [_vp, _vp, _u64p, _vp]),
    "blissgpu_ctx_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "blissgpu_ctx_destroy": (C.c_int, [_vp]),
    "blissgpu_ctx_set_stream": (C.c_int, [_vp, _vp]),
    "blissgpu_ctx_get_stream": (_vp, [_vp]),
    "blissgpu_ctx_wait_stream": (C.c_int, [_vp, _vp]),
    "blissgpu_ctx_signal_stream": (C.c_int, [_vp, _vp]),
    "blissgpu_ctx_set_workspace_limit": (C.c_int, [_vp, C.c_uint64]),
    "blissgpu_ctx_get_workspace_limit": (C.c_uint64, [_vp]),
    "blissgpu_ctx_synchronize": (C.c_int, [_vp]),
    "blissgpu_ctx_set_option": (C.c_int, [_vp, C.c_int, C.c_int64]),
    "blissgpu_ctx_staged_bytes": (C.c_uint64, [_vp]),
    "blissgpu_default_ctx": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "blissgpu_default_device_count": (C.c_int, []),
    "blissgpu_default_device": (C.c_int, [C.c_int]),
    "blissgpu_default_device_batches": (C.c_uint64, [C.c_int]),
    "blissgpu_set_single_song_timeout_ms": (C.c_int, [C.c_int64]),
    "blissgpu_default_reset": (C.c_int, []),
    "blissgpu_feature_count": (C.c_uint32, [C.c_uint32]),
    "blissgpu_analyze": (C.c_int, [_vp, C.c_uint64, C.c_uint32, _vp, _i32p]),
    "blissgpu_analyze_interleaved": (C.c_int, [_vp, C.c_int, C.c_uint32, C.c_uint64, C.c_uint32, _vp, _i32p]),
    "blissgpu_analyze_batch_interleaved": (C.c_int, [_vp, C.c_int, C.c_uint32, _u64p, _u64p, C.c_uint32, C.c_uint32, _vp, _i32p]),
    "blissgpu_pcm_downmix_device": (C.c_int, [_vp, _vp, C.c_int, C.c_uint32, C.c_uint64, _vp]),
    "blissgpu_debug_last_chunks": (C.c_uint64, [_vp]),
    "blissgpu_analyze_batch": (C.c_int, [_vp, _u64p, _u64p, C.c_uint32, C.c_uint32, _vp, _i32p]),
    "blissgpu_analyze_batch_s16": (C.c_int, [_vp, _u64p, _u64p, C.c_uint32, C.c_uint32, _vp, _i32p]),
    "blissgpu_pcm_s16_to_f32_device": (C.c_int, [_vp, _vp, C.c_uint64, _vp]),
    "blissgpu_host_alloc": (C.c_int, [C.POINTER(_vp), C.c_uint64]),
    "blissgpu_host_free": (C.c_int, [_vp]),
    "blissgpu_analyze_batch_device": (C.c_int, [_vp, _vp, _u64p, _u64p, C.c_uint32, C.c_uint32, _vp, _vp]),
    "blissgpu_distance": (C.c_int, [_vp, _vp, C.c_uint32, C.c_int, _vp, _f32p]),
    "blissgpu_pairwise": (C.c_int, [_vp, C.c_uint64, _vp, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp]),
    "blissgpu_pairwise_device": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp,
                                           C.c_uint64]),
    "blissgpu_set_distance": (C.c_int, [_vp, C.c_uint32, _vp, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp]),
    "blissgpu_closest_to_songs": (C.c_int, [_vp, C.c_uint32, _vp, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp, _vp]),
    "blissgpu_song_to_song": (C.c_int, [_vp, C.c_uint32, _vp, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp]),
    "blissgpu_dedup_playlist": (C.c_int, [_vp, C.c_uint64, C.c_uint32, _vp, C.c_uint64, _vp, C.c_int, _vp, C.c_float, _vp,
                                          _u64p]),
    "blissgpu_dedup_playlist_device": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint32, _vp, C.c_uint64, _vp, C.c_int, _vp,
                                                 C.c_float, _vp, _vp]),
    "blissgpu_knn": (C.c_int, [_vp, C.c_uint64, _vp, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp, C.c_uint32, _vp, _vp]),
    "blissgpu_knn_device": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp, C.c_uint32, _vp,
                                      _vp]),
    "blissgpu_scaled_knn": (C.c_int, [_vp, C.c_uint64, _vp, _vp, C.c_uint64, _vp, C.c_uint32, C.c_int, _vp, _vp, C.c_uint32, _vp,
                                      _vp]),
    "blissgpu_scaled_knn_device": (C.c_int, [_vp, _vp, C.c_uint64, _vp, _vp, C.c_uint64, _vp, C.c_uint32, C.c_int, _vp, _vp,
                                             C.c_uint32, _vp, _vp]),
    "blissgpu_knn_occurrence": (C.c_int, [_vp, C.c_uint64, C.c_uint32, C.c_uint64, _vp]),
    "blissgpu_knn_occurrence_device": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint32, C.c_uint64, _vp]),
    "blissgpu_kmeans": (C.c_int, [_vp, C.c_uint64, C.c_uint32, _vp, C.c_uint32, C.c_int, _vp, C.c_uint32, _vp, _vp, _vp, _vp,
                                  _u32p, _i32p]),
    "blissgpu_kmeans_device": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint32, _vp, C.c_uint32, C.c_int, _vp, C.c_uint32, _vp, _vp,
                                         _vp, _vp, _u32p, _i32p]),
    "blissgpu_debug_kmeans_stats": (C.c_int, [_vp, _u64p, _u64p]),
    "blissgpu_silhouette": (C.c_int, [_vp, C.c_uint64, C.c_uint32, _vp, C.c_uint32, C.c_int, _vp, _vp, C.c_uint64, C.c_uint32, _vp,
                                      _vp, _vp, _vp, _vp]),
    "blissgpu_silhouette_device": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint32, _vp, C.c_uint32, C.c_int, _vp, _vp, C.c_uint64,
                                             C.c_uint32, _vp, _vp, _vp, _vp, _vp]),
    "blissgpu_group_neighbours": (C.c_int, [_vp, C.c_uint64, C.c_uint32, _vp, C.c_uint32, C.c_int, _vp, _vp, C.c_uint64, C.c_uint32,
                                            C.c_int, C.c_uint32, _vp, _vp, _vp, _vp]),
    "blissgpu_group_neighbours_device": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint32, _vp, C.c_uint32, C.c_int, _vp, _vp, C.c_uint64,
                                                   C.c_uint32, C.c_int, C.c_uint32, _vp, _vp, _vp, _vp]),
    "blissgpu_mst": (C.c_int, [_vp, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "blissgpu_mst_device": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "blissgpu_ward_nearest": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp, _vp]),
    "blissgpu_ward": (C.c_int, [_vp, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "blissgpu_pam_scan": (C.c_int, [_vp, C.c_uint64, C.c_uint32, _vp, _vp, _vp, C.c_uint32, C.c_int, _vp, _vp, C.c_uint64, _vp, _vp, _vp,
                                    _vp, _vp]),
    "blissgpu_kmedoids": (C.c_int, [_vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp,
                                    _vp]),
    "blissgpu_pam_plan": (C.c_int, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_uint64, _vp]),
    "blissgpu_fingerprint_len": (C.c_uint64, [C.c_uint64]),
    "blissgpu_fingerprint_bands": (C.c_int, [_u32p]),
    "blissgpu_fingerprint_batch": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp]),
    "blissgpu_fingerprint_match": (C.c_int, [_vp, _vp, C.c_uint32, _vp, C.c_uint64, C.c_uint32, C.c_uint32, _vp, _vp, _vp]),
    "blissgpu_loudness_subblocks": (C.c_uint64, [C.c_uint64, C.c_uint32]),
    "blissgpu_loudness_kweighting": (C.c_int, [C.c_uint32, _f64p]),
    "blissgpu_true_peak_filter": (C.c_int, [C.c_uint32, _u32p, _f64p]),
    "blissgpu_loudness_blocks": (C.c_int, [_vp, C.c_uint32, C.c_uint64, C.c_uint32, _vp, _vp]),
    "blissgpu_loudness_gate": (C.c_int, [_vp, C.c_uint64, _f64p, _f64p]),
    "blissgpu_loudness_range": (C.c_int, [_vp, C.c_uint64, _f64p, _f64p, _f64p]),
    "blissgpu_loudness_energies": (C.c_int, [C.POINTER(DecodedSong), C.c_uint32, _vp, _vp, _vp, _i32p]),
    "blissgpu_loudness_batch": (C.c_int, [C.POINTER(DecodedSong), C.c_uint32, _vp, C.c_uint32, _vp, _vp, _i32p]),
    "blissgpu_moments": (C.c_int, [_vp, C.c_uint64, C.c_uint32, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "blissgpu_moments_device": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint32, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "blissgpu_covariance_metric": (C.c_int, [_vp, C.c_uint32, C.c_uint64, C.c_int, C.c_double, _vp, _i32p]),
    "blissgpu_triplet_step": (C.c_int, [_vp, C.c_uint64, C.c_uint32, _vp, C.c_uint64, _vp, C.c_double, _vp, _u64p, _f64p, _vp]),
    "blissgpu_triplet_step_device": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint32, _vp, C.c_uint64, _vp, C.c_double, _vp, _u64p,
                                               _f64p, _vp]),
    "blissgpu_learn_metric": (C.c_int, [_vp, C.c_uint64, C.c_uint32, _vp, C.c_uint64, C.c_int, _vp, C.c_double, C.c_double,
                                        C.c_double, C.c_uint32, _vp, _vp, _vp, _u32p, _u32p, _i32p]),
    "blissgpu_learn_metric_device": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint32, _vp, C.c_uint64, C.c_int, _vp, C.c_double,
                                               C.c_double, C.c_double, C.c_uint32, _vp, _vp, _vp, _u32p, _u32p, _i32p]),
    "blissgpu_debug_metric_stats": (C.c_int, [_vp, _u64p, _u64p, _u64p]),
    "blissgpu_group_knn": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp, C.c_uint32, _vp,
                                     _vp]),
    "blissgpu_group_knn_device": (C.c_int, [_vp, _vp, _vp, C.c_uint64, _vp, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp,
                                            C.c_uint32, _vp, _vp]),
    "blissgpu_group_knn_plan": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, _vp, C.c_uint64, _u64p, _u32p,
                                          _u32p]),
    "blissgpu_group_weights": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint32, _vp, _vp]),
    "blissgpu_group_weights_device": (C.c_int, [_vp, _vp, _vp, C.c_uint64, C.c_uint32, _vp, _vp]),
    "blissgpu_group_knn_weighted": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint64, C.c_uint32, _vp, _vp, C.c_uint32, _vp, _vp,
                                              _vp]),
    "blissgpu_group_knn_weighted_device": (C.c_int, [_vp, _vp, _vp, C.c_uint64, _vp, C.c_uint64, C.c_uint32, _vp, _vp,
                                                     C.c_uint32, _vp, _vp, _vp]),
    "blissgpu_album_knn": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint64, C.c_uint32, _vp, C.c_uint64, _vp, C.c_uint32, _vp, _vp,
                                     _vp, _vp]),
    "blissgpu_album_knn_device": (C.c_int, [_vp, _vp, _vp, C.c_uint64, _vp, C.c_uint64, C.c_uint32, _vp, C.c_uint64, _vp,
                                            C.c_uint32, _vp, _vp, _vp, _vp]),
    "blissgpu_chains": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp, C.c_uint32, C.c_int, _vp,
                                  _vp]),
    "blissgpu_chains_device": (C.c_int, [_vp, _vp, _vp, C.c_uint64, _vp, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp, C.c_uint32,
                                         C.c_int, _vp, _vp]),
    "blissgpu_chains_plan": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.POINTER(C.c_int), _u32p]),
    "blissgpu_journeys": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp, C.c_uint32, C.c_int, C.c_int,
                                    C.c_uint32, _vp, _vp]),
    "blissgpu_journeys_device": (C.c_int, [_vp, _vp, _vp, C.c_uint64, _vp, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp, C.c_uint32,
                                           C.c_int, C.c_int, C.c_uint32, _vp, _vp]),
    "blissgpu_radio": (C.c_int, [_vp, C.c_uint64, _vp, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp,
                                 C.c_uint32, C.c_int, _vp, _vp]),
    "blissgpu_radio_device": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp, _vp, C.c_uint32, _vp,
                                        _vp, _vp, C.c_uint32, C.c_int, _vp, _vp]),
    "blissgpu_map_step": (C.c_int, [_vp, C.c_uint64, _vp, _vp, _vp, C.c_float, C.c_uint32, _vp, _vp, _vp]),
    "blissgpu_map_layout": (C.c_int, [_vp, C.c_uint64, _vp, _vp, _vp, C.c_uint32, C.c_uint32, C.c_float, C.c_double, C.c_double,
                                      C.c_double, C.c_double, C.c_uint32, _vp, _vp]),
    "blissgpu_map_plan": (C.c_int, [C.c_uint64, C.c_uint32, _u32p]),
    "blissgpu_duplicate_groups": (C.c_int, [_vp, C.c_uint64, C.c_uint32, _vp, C.c_int, _vp, C.c_float, _vp, _u64p, _vp, _vp,
                                            C.c_uint64]),
    "blissgpu_duplicate_groups_device": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint32, _vp, C.c_int, _vp, C.c_float, _vp, _vp, _vp,
                                                   _vp, C.c_uint64]),
    "blissgpu_forest_build": (C.c_int, [_vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                        C.POINTER(_vp)]),
    "blissgpu_forest_destroy": (C.c_int, [_vp]),
    "blissgpu_forest_info": (C.c_int, [_vp, _u32p, _u32p, _u32p, _u32p, _u32p, _u64p]),
    "blissgpu_forest_export": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "blissgpu_forest_score": (C.c_int, [_vp, _vp, C.c_uint64, _vp, _vp]),
    "blissgpu_forest_closest_to_songs": (C.c_int, [_vp, _vp, C.c_uint64, _vp, _vp]),
    "blissgpu_forest_score_device": (C.c_int, [_vp, _vp, _vp, C.c_uint64, _vp, _vp]),
    "blissgpu_forest_closest_to_songs_device": (C.c_int, [_vp, _vp, _vp, C.c_uint64, _vp, _vp]),
    "blissgpu_group_forest_knn": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                            C.c_uint32, C.c_uint64, _vp, C.c_uint32, _vp, _vp, _vp]),
    "blissgpu_group_forest_knn_device": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint64, _vp, C.c_uint64, C.c_uint32, C.c_uint32,
                                                   C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, _vp, C.c_uint32, _vp, _vp, _vp]),
    "blissgpu_group_forest_plan": (C.c_int, [_vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                             C.c_uint64, _vp, C.c_uint64, _u64p]),
    "blissgpu_debug_group_forest_stats": (C.c_int, [_vp, _f64p, _f64p, _u64p]),
    "blissgpu_set_distance_device": (C.c_int, [_vp, _vp, C.c_uint32, _vp, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp]),
    "blissgpu_closest_to_songs_device": (C.c_int, [_vp, _vp, C.c_uint32, _vp, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp,
                                                   _vp]),
    "blissgpu_song_to_song_device": (C.c_int, [_vp, _vp, C.c_uint32, _vp, C.c_uint64, C.c_uint32, C.c_int, _vp, _vp]),
    "blissgpu_shard_plan": (C.c_int, [_u64p, C.c_uint32, C.c_uint32, _u32p]),
    "blissgpu_row_block": (None, [C.c_uint64, C.c_uint32, C.c_uint32, _u64p, _u64p]),
    "blissgpu_node_create": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(_vp)]),
    "blissgpu_node_destroy": (C.c_int, [_vp]),
    "blissgpu_node_device_count": (C.c_int, [_vp]),
    "blissgpu_node_ctx": (_vp, [_vp, C.c_int]),
    "blissgpu_node_shard": (C.c_int, [_vp, _u64p, C.c_uint32, _u32p]),
    "blissgpu_node_row_block": (None, [_vp, C.c_uint64, C.c_int, _u64p, _u64p]),
    "blissgpu_node_analyze": (C.c_int, [_vp, _vp, _u64p, _u64p, C.c_uint32, C.c_uint32, _vp, _i32p]),
    "blissgpu_node_analyze_device": (C.c_int, [_vp, C.POINTER(_vp), _u64p, _u64p, _u32p, C.c_uint32, C.c_uint32]),
    "blissgpu_node_features": (_vp, [_vp, C.c_int]),
    "blissgpu_node_pairwise": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "blissgpu_node_synchronize": (C.c_int, [_vp]),
    "blissgpu_feature_weights": (C.c_int, [C.c_uint32, _vp]),
    "blissgpu_malloc": (C.c_int, [C.POINTER(_vp), C.c_uint64]),
    "blissgpu_free": (C.c_int, [_vp]),
    "blissgpu_memcpy_h2d": (C.c_int, [_vp, _vp, _vp, C.c_uint64]),
    "blissgpu_memcpy_d2h": (C.c_int, [_vp, _vp, _vp, C.c_uint64]),
    "blissgpu_synth_white_noise_device": (C.c_int, [_vp, _vp, _u64p, _u64p, C.c_uint32, C.c_uint32]),
    "blissgpu_synth_white_noise_indexed_device": (C.c_int, [_vp, _vp, _u64p, _u64p, _u32p, C.c_uint32]),
    "blissgpu_profile_enable": (C.c_int, [_vp, C.c_int]),
    "blissgpu_profile_reset": (C.c_int, [_vp]),
    "blissgpu_profile_kernel_count": (C.c_int, []),
    "blissgpu_profile_kernel_name": (C.c_char_p, [C.c_int]),
    "blissgpu_profile_get": (C.c_int, [_vp, C.c_int, _f64p, _u64p]),
    "blissgpu_debug_last_tuning": (C.c_int, [_vp, _f64p, _u32p, C.c_uint32]),
    "blissgpu_debug_fetch": (C.c_int, [_vp, C.c_int, C.c_uint32, _vp, C.c_uint64, _u64p]),
    "blissgpu_strerror": (C.c_char_p, [C.c_int]),
    "blissgpu_last_error": (C.c_char_p, []),
    "blissgpu_version": (C.c_char_p, []),
}

_lib = None


class BlissGpuError(RuntimeError):
    def __init__(self, code, detail):
        super().__init__(f"blissgpu error {code}: {detail}")
        self.code = code


def lib():
    """Load libblissgpu.so (fails loudly when the HIP extension has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        try:  # share torch's HIP runtime instance when torch is around (same SONAME libamdhip64.so.7)
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch is optional for the C ABI
            pass
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != OK:
        L = lib()
        detail = L.blissgpu_last_error().decode() or L.blissgpu_strerror(rc).decode()
        raise BlissGpuError(rc, detail)


# the c_int results that are values, not a status
_INT_VALUES = frozenset({"blissgpu_default_device_count", "blissgpu_default_device", "blissgpu_node_device_count",
                         "blissgpu_profile_kernel_count"})


def _pointer(name, pos, a, argtype):
    """The C argument for the numpy array or torch tensor `a` at position `pos` of `name`: its address, once it is known to
    be C-contiguous and, for a typed pointer argtype, of the pointee's dtype."""
    is_array = isinstance(a, np.ndarray)
    if not (a.flags.c_contiguous if is_array else a.is_contiguous()):
        raise TypeError(f"{name}: argument {pos} is not C-contiguous")
    if not is_array:
        return C.c_void_p(a.data_ptr())
    if argtype is _vp:
        return a.ctypes.data  # (the plain address: what a `void *` argument has always been given here)
    want = np.dtype(argtype._type_)
    if (a.dtype.kind, a.dtype.itemsize) != (want.kind, want.itemsize):
        raise TypeError(f"{name}: argument {pos} is {a.dtype}, the C argument points to {want}")
    return a.ctypes.data_as(argtype)


def address(a) -> int:
    """the address of a C-contiguous numpy array, for the two places an address is data and not an argument: a pointer
    table and the `pcm` field of DecodedSong.  The caller keeps the array alive across the call."""
    if not a.flags.c_contiguous:
        raise TypeError("an array whose address is handed to the library must be C-contiguous")
    return a.ctypes.data


def pointer_table(arrays):
    """`void *table[n]` of the arrays' addresses (blissgpu_*_flac*: one file or one output buffer per song)"""
    return (C.c_void_p * len(arrays))(*[address(a) for a in arrays])


_ndarray = np.ndarray
_PLAIN = frozenset({int, float, bool, type(None)})  # what most arguments are: passed on without a further look
_status = {name: res is C.c_int and name not in _INT_VALUES for name, (res, _) in SIGNATURES.items()}  # returns a status?


def _arguments(name, args, argtypes):
    """(the second line is _pointer's commonest case, a contiguous array for a `void *`, without the call)"""
    return [a if (t := type(a)) in _PLAIN else
            a.ctypes.data if t is _ndarray and argtypes[i] is _vp and a.flags.c_contiguous else
            _pointer(name, i, a, argtypes[i]) if isinstance(a, _ndarray) or hasattr(a, "data_ptr") else a
            for i, a in enumerate(args)]


def call_unchecked(name, *args):
    """`name`(*args) in the library -- the one place a Python object becomes a C argument.  None, Python scalars and ctypes
    objects pass as they are; a numpy array or a torch tensor becomes its address (`_pointer`: a TypeError instead of a call
    for a strided array or the wrong dtype).  `args` keeps every array and tensor alive until the function has returned.
    The function is looked up in lib() at every call: the tests replace lib() or single functions of the library.
    -> what the function returned."""
    return getattr(lib(), name)(*_arguments(name, args, SIGNATURES[name][1]))


def call(name, *args):
    """call_unchecked, then check() for the functions that return a status; the others return their value."""
    out = getattr(lib(), name)(*_arguments(name, args, SIGNATURES[name][1]))
    if not _status[name]:
        return out
    if out != OK:
        check(out)
