"""ctypes binding of include/dcs_hip.h.  Fails loudly when the shared library is missing: there is
no Python or CPU implementation of the decode path in this package."""
import ctypes
import os
import weakref

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

OS93A, OS93B, OS94, OS95 = 0, 1, 2, 3
ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_NO_MEMORY, ERR_CAPACITY, ERR_BAD_STREAM = -1, -2, -3, -4, -5, -6
FMT_93_T0, FMT_93B_T1, FMT_93A_T1, FMT_94_T0, FMT_94_T1_S0, FMT_94_T1_S3 = range(6)
FRAME_SAMPLES = 240
FRAME_STOP, FRAME_FATAL, FRAME_TAIL_LOST = 1, 2, 4
PREV_NONE = 0xFFFFFFFF
PREV_EXT = 0x80000000
XFORM_93, XFORM_94 = 0, 1

# numpy views of the ABI structs (layouts asserted against the library at load time)
SPLIT_DTYPE = np.dtype([("bitDelta", "<u2"), ("prv", "<u2"), ("prvDelta", "<u2"), ("state", "<u2")])
INDEX_DTYPE = np.dtype([("bitOff", "<u4"), ("nBits", "<u2"), ("hdrBits", "<u2"), ("bandType", "u1", (16,)),
                        ("preAdj", "<u2"), ("nBands", "u1"), ("flags", "u1"), ("split", SPLIT_DTYPE, (15,))])
SRC_DTYPE = np.dtype([("streamOff", "<u8"), ("mixMul", "<u2"), ("format", "u1"), ("hdrLen", "u1"),
                      ("idx", INDEX_DTYPE)])
JOB_DTYPE = np.dtype([("firstSrc", "<u4"), ("nSrc", "u1"), ("volShift", "u1"), ("xform", "u1"), ("flags", "u1"),
                      ("prev", "<u4"), ("reserved", "<u4")])
assert SRC_DTYPE.itemsize == 160 and JOB_DTYPE.itemsize == 16 and INDEX_DTYPE.itemsize == 148
IDX_SERIAL = 1


class StreamInfo(ctypes.Structure):
    _fields_ = [("nFrames", ctypes.c_int32), ("nBytes", ctypes.c_int32), ("formatType", ctypes.c_int32),
                ("formatSubType", ctypes.c_int32), ("header", ctypes.c_uint8 * 16), ("format", ctypes.c_int32),
                ("hdrLen", ctypes.c_int32), ("nValidFrames", ctypes.c_int32), ("payloadBits", ctypes.c_uint32)]


class StreamRef(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("len", ctypes.c_size_t), ("os", ctypes.c_int32),
                ("volume", ctypes.c_int32), ("level", ctypes.c_int32), ("channelVolume", ctypes.c_int32)]


LOC_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("os", "<i4"), ("firstRecord", "<u8")])
INFO_DTYPE = np.dtype([("nFrames", "<i4"), ("nBytes", "<i4"), ("formatType", "<i4"), ("formatSubType", "<i4"),
                       ("header", "u1", (16,)), ("format", "<i4"), ("hdrLen", "<i4"), ("nValidFrames", "<i4"),
                       ("payloadBits", "<u4")])


class RomCheck(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("hw", ctypes.c_int32), ("os", ctypes.c_int32),
                ("nominalVersion", ctypes.c_uint32), ("catalogOffset", ctypes.c_uint32), ("nTracks", ctypes.c_uint32),
                ("signature", ctypes.c_char * 128)]


class TrackInfo(ctypes.Structure):
    _fields_ = [("address", ctypes.c_uint32), ("channel", ctypes.c_int32), ("type", ctypes.c_int32),
                ("deferCode", ctypes.c_int32), ("time", ctypes.c_uint32), ("looping", ctypes.c_int32)]


TRACKOP_DTYPE = np.dtype([("offset", "<i4"), ("nestingLevel", "<i4"), ("loopParent", "<i4"), ("delayCount", "<u2"),
                          ("opcode", "u1"), ("nOperandBytes", "u1"), ("operandBytes", "u1", (8,))])
EXTRACT_DTYPE = np.dtype([("track", "<u4"), ("streamNum", "<u4"), ("address", "<u4"), ("level", "<i4")])
HW_DCS93, HW_DCS95 = 2, 3


class PipelineResult(ctypes.Structure):
    _fields_ = [("pcm", ctypes.c_void_p), ("err", ctypes.c_void_p), ("frameOffsets", ctypes.c_void_p),
                ("nFrames", ctypes.c_uint32), ("nStreams", ctypes.c_uint32), ("status", ctypes.c_int32),
                ("hostMs", ctypes.c_float), ("deviceMs", ctypes.c_float), ("path", ctypes.c_uint32)]


# DcsPipelineFlacResult: what dcs_pipeline_collect_flac fills for a list of a FLAC pipeline (PIPE_FLAC, PIPE_FLAC_MD5)
PIPE_FLAC, PIPE_FLAC_MD5 = 8, 16


class PipelineFlacResult(ctypes.Structure):
    _fields_ = [("flac", ctypes.c_void_p), ("flacOffsets", ctypes.c_void_p), ("info", ctypes.c_void_p), ("err", ctypes.c_void_p),
                ("frameOffsets", ctypes.c_void_p), ("nFrames", ctypes.c_uint32), ("nStreams", ctypes.c_uint32),
                ("status", ctypes.c_int32), ("hostMs", ctypes.c_float), ("deviceMs", ctypes.c_float), ("path", ctypes.c_uint32)]


class DevicePathTimes(ctypes.Structure):
    _fields_ = [("passMs", ctypes.c_float), ("indexMs", ctypes.c_float), ("planMs", ctypes.c_float), ("packMs", ctypes.c_float),
                ("decodeMs", ctypes.c_float), ("planFlags", ctypes.c_uint32), ("nStreams", ctypes.c_uint32), ("nFrames", ctypes.c_uint32),
                ("framesPerWave", ctypes.c_uint32), ("algorithmicBytes", ctypes.c_uint64)]


class EncodeParams(ctypes.Structure):
    _fields_ = [("formatVersion", ctypes.c_uint16), ("reserved", ctypes.c_uint16), ("streamFormatType", ctypes.c_int32),
                ("streamFormatSubType", ctypes.c_int32), ("powerBandCutoff", ctypes.c_float), ("targetBitRate", ctypes.c_int32),
                ("minimumDynamicRange", ctypes.c_float), ("maximumQuantizationError", ctypes.c_float)]


class Budget(ctypes.Structure):
    """DcsBudget: what the budget calls on any source hold their jobs to (_budget builds one)"""
    _fields_ = [("budgetBytes", ctypes.c_void_p), ("totalBytes", ctypes.c_uint64), ("capBytes", ctypes.c_void_p),
                ("shared", ctypes.c_uint32), ("fit", ctypes.c_void_p)]


FILES_REENCODE_ALL = 0x100
ENCODE_INFO_DTYPE = np.dtype([("formatType", "<i4"), ("formatSubType", "<i4"), ("nFrames", "<i4"), ("nBytes", "<i4"),
                              ("bandsToKeep", "<i4")])
# the layouts encode_streams can be asked for: (type, sub-type); None = the reference's wildcard (-1, -1)
FMT_94_T0_S3 = "94-T0-S3"
_ENCODE_FMT = {None: (-1, -1), FMT_94_T0: (0, 0), FMT_94_T1_S0: (1, 0), FMT_94_T1_S3: (1, 3), FMT_94_T0_S3: (0, 3)}


# dcs_encode_sweep: a job's record (DcsSweepResult), the job list's entries (DcsSweepJob) and the flag that measures
SWEEP_RESULT_DTYPE = np.dtype([("enc", ENCODE_INFO_DTYPE), ("measured", "<u4"), ("peakErr", "<i4"), ("nCompared", "<u8"),
                               ("sumSrcSq", "<i8"), ("sumDecSq", "<i8"), ("sumCross", "<i8")], align=True)
SWEEP_JOB_DTYPE = np.dtype([("stream", "<u4"), ("paramSet", "<u4")])
SWEEP_MEASURE = 1


# dcs_transcode_*: what happens to a source, and its record (DcsTranscodeInfo)
TRANSCODE_COPIED, TRANSCODE_REENCODED = 0, 1
TRANSCODE_REENCODE_ALL = 1
TRANSCODE_INFO_DTYPE = np.dtype([("action", "<i4"), ("srcFrames", "<i4"), ("enc", ENCODE_INFO_DTYPE)])
# a target format version -> the OS its streams play under (and the DCSa container names)
TRANSCODE_OS = {0x9301: 0, 0x9302: 1, 0x9400: 2}


# dcs_resample_*: libsamplerate's coefficient layout, and the flag that runs the converter at 31 250 Hz too
class ResampleFilter(ctypes.Structure):
    _fields_ = [("coeffs", ctypes.c_void_p), ("nCoeffs", ctypes.c_int32), ("increment", ctypes.c_int32)]


RESAMPLE_AT_UNITY = 1


# dcs_wav_parse / dcs_encode_files: the reader's record of one WAV file, and what each file became
class WavInfo(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("formatCode", ctypes.c_int32), ("sampleFormat", ctypes.c_int32),
                ("bitDepth", ctypes.c_int32), ("channels", ctypes.c_int32), ("rate", ctypes.c_uint32),
                ("blockAlign", ctypes.c_int32), ("reserved", ctypes.c_int32), ("dataOffset", ctypes.c_uint64),
                ("dataSize", ctypes.c_uint64), ("nValues", ctypes.c_uint64), ("nBlocks", ctypes.c_uint64),
                ("reason", ctypes.c_char * 96)]


WAV_U8, WAV_S16, WAV_S24, WAV_S32, WAV_F32, WAV_F64, WAV_IMA, WAV_S8 = range(8)
FILE_WAV, FILE_DCSA_COPY, FILE_DCSA_REENCODE, FILE_FLAC = 0, 1, 2, 3
FILE_WALK_NONE, FILE_WALK_DEVICE, FILE_WALK_HOST = 0, 1, 2
ENCODE_FILE_INFO_DTYPE = np.dtype([("kind", "<i4"), ("sourceFormat", "<i4"), ("rate", "<u4"), ("channels", "<i4"),
                                   ("nValues", "<u8"), ("nSamples", "<u8"), ("walk", "<i4"), ("srcFrames", "<i4"),
                                   ("enc", ENCODE_INFO_DTYPE)], align=True)


# dcs_flac_parse / dcs_flac_index: the reader's record of one FLAC file and of each of its frames
class FlacInfo(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("rate", ctypes.c_uint32), ("channels", ctypes.c_int32), ("bitDepth", ctypes.c_int32),
                ("sampleFormat", ctypes.c_int32), ("minBlockSize", ctypes.c_uint32), ("maxBlockSize", ctypes.c_uint32),
                ("nFrames", ctypes.c_uint32), ("totalSamples", ctypes.c_uint64), ("nValues", ctypes.c_uint64),
                ("firstFrameOffset", ctypes.c_uint64), ("reason", ctypes.c_char * 96)]


FLAC_FRAME_DTYPE = np.dtype([("offset", "<u8"), ("length", "<u4"), ("blockSize", "<u4"), ("firstSample", "<u8"),
                             ("channelAssignment", "<i4"), ("bitsPerSample", "<i4"), ("blockingStrategy", "<i4"),
                             ("headerLength", "<i4")], align=True)


# dcs_flac_write_streams, dcs_decode_streams_flac: flags, and what was written per stream
FLAC_MD5 = 1
FLAC_SEQUENCE = 2
FLAC_AT_UNITY = 4               # dcs_decode_streams_flac_at only: RESAMPLE_AT_UNITY for its converter
FLAC_WRITE_INFO_DTYPE = np.dtype([("nSamples", "<u8"), ("nBytes", "<u8"), ("nBlocks", "<u4"), ("nConstant", "<u4"), ("nVerbatim", "<u4"),
                                  ("nFixed", "<u4"), ("minFrame", "<u4"), ("maxFrame", "<u4")], align=True)

# dcs_resample_out_streams, dcs_decode_streams_at: the decode call's flag, and what the converter made of each stream
OUT_SEQUENCE = 2
RATE_INFO_DTYPE = np.dtype([("nIn", "<u8"), ("nOut", "<u8"), ("nClipped", "<u8"), ("peak", "<f4"), ("reserved", "<u4")], align=True)


# dcs_level_*: what happens to a stream's level between the converter and the encoder, and what the stage did
class Level(ctypes.Structure):
    """DcsLevel.  Level(LEVEL_FIT, ceiling=1.0), Level(LEVEL_GAIN, gain=0.5), Level(LEVEL_GAIN, LEVEL_CLIP, 2.0, 0.9)"""
    _fields_ = [("mode", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("gain", ctypes.c_float), ("ceiling", ctypes.c_float)]

    def __init__(self, mode=0, flags=0, gain=1.0, ceiling=1.0):
        super().__init__(mode, flags, gain, ceiling)


LEVEL_GAIN, LEVEL_FIT, LEVEL_NORMALIZE = 1, 2, 3
LEVEL_CLIP = 1
LEVEL_INFO_DTYPE = np.dtype([("peakIn", "<f4"), ("gain", "<f4"), ("peakOut", "<f4"), ("mode", "<u4"), ("nClipped", "<u8")], align=True)


class SynthParams(ctypes.Structure):
    _fields_ = [("seed", ctypes.c_uint64), ("format", ctypes.c_int32), ("nFrames", ctypes.c_int32),
                ("nBands", ctypes.c_int32), ("strideFromBand", ctypes.c_int32), ("profile", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


def _view(ptr, ctype, dtype, shape):
    """a numpy view of library memory (np.ctypeslib.as_array costs 0.6 ms per call for a 15 M-element array)"""
    addr = ptr.value if isinstance(ptr, ctypes.c_void_p) else ptr
    n = 1
    for d in shape:
        n *= int(d)
    if n == 0 or not addr:
        return np.zeros(shape, dtype=dtype)
    return np.frombuffer((ctype * n).from_address(addr), dtype=dtype).reshape(shape)


class DcsError(RuntimeError):
    def __init__(self, status, msg=""):
        super().__init__("libdcs_hip status %d %s" % (status, msg))
        self.status = status


_LIB = None
ABI_VERSION = 9                 # include/dcs_hip.h DCS_ABI_VERSION these bindings are written for

EXPORTS = [
    "dcs_index_stream_mids", "dcs_index_streams_mids", "dcs_batch_create_mids", "dcs_ctx_set_even_deal", "dcs_batch_even_deal",
    "dcs_pack_chunks_mids", "dcs_even_deal_lane", "dcs_ctx_set_sole_source_kernel", "dcs_batch_sole_source_kernel",
    "dcs_batch_filled_bands", "dcs_prepass_short",
    "dcs_abi_version", "dcs_build_id", "dcs_index_stream", "dcs_volume_multiplier", "dcs_mixing_multiplier", "dcs_frame_scale",
    "dcs_stream_params", "dcs_ctx_create", "dcs_ctx_destroy", "dcs_last_error", "dcs_device_count", "dcs_runtime_defaults", "dcs_ctx_set_batch_tails", "dcs_batch_package_bytes",
    "dcs_ctx_set_frames_per_wave", "dcs_ctx_set_tail_handoff", "dcs_ctx_set_large_list_path", "dcs_ctx_set_concurrent_batches", "dcs_ctx_set_cache_limits", "dcs_ctx_trim_cache", "dcs_ctx_cache_bytes", "dcs_plan_chunks2", "dcs_decode_batch", "dcs_batch_create", "dcs_batch_destroy", "dcs_batch_run", "dcs_batch_run_many", "dcs_pack_chunks",
    "dcs_batch_time", "dcs_batch_time_rotating", "dcs_batch_sync", "dcs_batch_download", "dcs_batch_download_view", "dcs_batch_device_pcm",
    "dcs_batch_algorithmic_bytes", "dcs_batch_num_jobs", "dcs_decode_streams", "dcs_count_stream_frames",
    "dcs_synth_stream", "dcs_plan_chunks", "dcs_index_streams", "dcs_index_streams_gpu",
    "dcs_index_streams_gpu_time", "dcs_stream_params_from", "dcs_decode_stream_sequence", "dcs_wav_header",
    "dcs_dcsa_header", "dcs_dcsa_parse", "dcs_write_wav", "dcs_write_dcsa", "dcs_frame_diff",
    "dcs_romset_create", "dcs_romset_destroy", "dcs_romset_last_error", "dcs_romset_add_rom", "dcs_romset_load_zip",
    "dcs_romset_load_zip_memory", "dcs_romset_check", "dcs_romset_set_version", "dcs_romset_num_tracks",
    "dcs_romset_pointer", "dcs_romset_bytes_behind", "dcs_romset_track_info", "dcs_romset_decompile", "dcs_romset_list_streams",
    "dcs_romset_extract_plan", "dcs_romset_stream_refs", "dcs_romset_extract_tracks_plan", "dcs_extract_tracks",
    "dcs_seq_create", "dcs_seq_destroy", "dcs_seq_last_error", "dcs_seq_set_master_volume", "dcs_seq_set_reported_version",
    "dcs_seq_write_data_port", "dcs_seq_add_track_command", "dcs_seq_clear_tracks", "dcs_seq_load_audio_stream",
    "dcs_seq_plan", "dcs_seq_pending_ticks", "dcs_seq_is_fatal", "dcs_seq_host_bytes", "dcs_seq_decode",
    "dcs_seq_create_standalone", "dcs_seq_load_audio_stream_mem", "dcs_seq_rewind", "dcs_seq_set_rewindable",
    "dcs_seq_tick", "dcs_seq_fatal_tick", "dcs_seq_stream_playing",
    "dcs_decode_batch_live", "dcs_seq_decode_view", "dcs_seq_plan_ahead", "dcs_seq_stream_playing_at", "dcs_seq_tracks_active_at", "dcs_ctx_call_floor",
    "dcs_host_threads", "dcs_partition_streams", "dcs_decode_streams_sharded",
    "dcs_ctx_set_frames_per_chunk", "dcs_index_stream_literal", "dcs_pack_chunks_device", "dcs_batch_abi_bytes", "dcs_batch_num_chunks", "dcs_batch_frames_per_wave", "dcs_ctx_set_chunks_per_wave", "dcs_batch_chunks_per_wave", "dcs_ctx_clock_mhz", "dcs_ctx_link_rate", "dcs_ctx_set_test_hooks",
    "dcs_pipeline_create", "dcs_pipeline_destroy", "dcs_pipeline_submit", "dcs_pipeline_collect", "dcs_pipeline_collect_flac",
    "dcs_device_path_create", "dcs_device_path_run", "dcs_device_path_run_many", "dcs_device_path_download", "dcs_device_path_destroy",
    "dcs_node_create", "dcs_node_destroy", "dcs_node_submit", "dcs_node_collect", "dcs_node_num_devices", "dcs_node_device_info",
    "dcs_node_last_error", "dcs_node_cache_release", "dcs_device_numa_node",
    "dcs_encode_params_default", "dcs_encode_bound", "dcs_encode_header", "dcs_encode_streams",
    "dcs_encode93_bound", "dcs_encode93_header", "dcs_encode93_streams",
    "dcs_encode93a_bound", "dcs_encode93a_streams", "dcs_encode93a_sweep",
    "dcs_encode_rd_bound", "dcs_encode_rd_streams", "dcs_encode93_rd_bound", "dcs_encode93_rd_streams",
    "dcs_encode_rd_fit", "dcs_encode93_rd_fit", "dcs_encode_rd_allot",
    "dcs_transcode_plan", "dcs_transcode_streams",
    "dcs_resample_filter_default", "dcs_resample_count", "dcs_resample_streams", "dcs_encode_streams_at",
    "dcs_wav_parse", "dcs_encode_files_plan", "dcs_wav_decode", "dcs_encode_files",
    "dcs_flac_parse", "dcs_flac_index", "dcs_flac_decode",
    "dcs_flac_write_bound", "dcs_flac_write_check", "dcs_flac_write_streams", "dcs_decode_streams_flac",
    "dcs_encode_sweep", "dcs_encode_sweep_group_frames", "dcs_encode_fit",
    "dcs_level_gain", "dcs_level_streams", "dcs_resample_streams_level", "dcs_encode_streams_at_level", "dcs_encode_files_level",
    "dcs_resample_out_count", "dcs_resample_out_walk", "dcs_resample_out_streams", "dcs_decode_streams_at",
    "dcs_flac_write_samples_check", "dcs_flac_write_samples", "dcs_decode_streams_flac_at",
    "dcs_encode_streams_at_budget", "dcs_transcode_plan_budget", "dcs_transcode_streams_budget", "dcs_encode_files_plan_budget",
    "dcs_encode_files_budget",
]


def build_id():
    """the digest of sources and flags the LOADED library was built from (dcs_build_id)"""
    return load_library().dcs_build_id().decode()


def lib_sha256():
    import hashlib
    return hashlib.sha256(open(lib_path(), "rb").read()).hexdigest()


def lib_path():
    # DCS_HIP_LIB: another build of the same library (kernel A/B comparisons, tools/ab.sh); never a different backend
    return os.environ.get("DCS_HIP_LIB") or os.path.join(HERE, "libdcs_hip.so")


def load_library():
    """Load libdcs_hip.so.  If torch is importable it is imported first so that the process uses a
    single HIP runtime (torch bundles its own libamdhip64 with the same soname)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise ImportError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C dcsexplorer_amd/csrc` (there is no fallback implementation)" % path)
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = ctypes.CDLL(path)
    vp, u32, i32, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_size_t
    L.dcs_abi_version.restype = u32
    L.dcs_build_id.restype = ctypes.c_char_p
    if L.dcs_abi_version() != ABI_VERSION:
        # (DCS_HIP_LIB may name another BUILD of this library, tools/ab.sh; one with other struct layouts must not be driven
        # through these bindings: dcs_pipeline_collect writes sizeof(DcsPipelineResult) bytes into the caller's struct)
        raise ImportError("%s has ABI version %d, these bindings are written for %d: rebuild it (make -C dcsexplorer_amd/csrc)"
                          % (path, L.dcs_abi_version(), ABI_VERSION))
    L.dcs_index_stream.restype = i32
    L.dcs_index_stream.argtypes = [i32, vp, sz, vp, u32, ctypes.POINTER(StreamInfo)]
    L.dcs_index_stream_literal.restype = i32
    L.dcs_index_stream_literal.argtypes = [i32, vp, sz, vp, u32, ctypes.POINTER(StreamInfo)]
    L.dcs_volume_multiplier.restype = ctypes.c_uint16
    L.dcs_volume_multiplier.argtypes = [ctypes.c_int]
    L.dcs_mixing_multiplier.restype = ctypes.c_uint16
    L.dcs_mixing_multiplier.argtypes = [i32, ctypes.c_int, ctypes.c_int]
    L.dcs_frame_scale.restype = ctypes.c_int
    L.dcs_frame_scale.argtypes = [ctypes.c_uint16, vp, vp, ctypes.c_int]
    L.dcs_stream_params.restype = i32
    L.dcs_stream_params.argtypes = [i32, ctypes.c_int, ctypes.c_int, ctypes.c_int, u32, vp, vp]
    L.dcs_ctx_create.restype = i32
    L.dcs_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.dcs_ctx_destroy.restype = None
    L.dcs_ctx_destroy.argtypes = [vp]
    L.dcs_last_error.restype = ctypes.c_char_p
    L.dcs_last_error.argtypes = [vp]
    L.dcs_device_count.restype = ctypes.c_int
    L.dcs_ctx_set_frames_per_wave.restype = i32
    L.dcs_ctx_set_frames_per_wave.argtypes = [vp, ctypes.c_int]
    if hasattr(L, "dcs_ctx_set_chunks_per_wave"):       # (DCS_HIP_LIB may name a build from before there was the setting: A/B against it)
        L.dcs_ctx_set_chunks_per_wave.restype = i32
        L.dcs_ctx_set_chunks_per_wave.argtypes = [vp, ctypes.c_int]
    L.dcs_ctx_set_tail_handoff.restype = i32
    L.dcs_ctx_set_tail_handoff.argtypes = [vp, ctypes.c_int]
    L.dcs_ctx_set_large_list_path.restype = i32
    L.dcs_ctx_set_large_list_path.argtypes = [vp, ctypes.c_int]
    L.dcs_ctx_set_concurrent_batches.restype = i32
    L.dcs_ctx_set_concurrent_batches.argtypes = [vp, ctypes.c_int]
    u64p = ctypes.POINTER(ctypes.c_uint64)
    L.dcs_ctx_set_cache_limits.restype = i32
    L.dcs_ctx_set_cache_limits.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint64]
    L.dcs_ctx_trim_cache.restype = i32
    L.dcs_ctx_trim_cache.argtypes = [vp, u64p, u64p]
    L.dcs_ctx_cache_bytes.restype = i32
    L.dcs_ctx_cache_bytes.argtypes = [vp, u64p, u64p, u64p, u64p]
    L.dcs_pack_chunks.restype = i32
    L.dcs_pack_chunks.argtypes = [vp, u32, vp, vp, sz, ctypes.c_int, vp, sz, ctypes.POINTER(u32), ctypes.POINTER(u32)]
    L.dcs_plan_chunks2.restype = i32
    L.dcs_plan_chunks2.argtypes = [vp, u32, vp, ctypes.c_int, ctypes.c_int, vp, sz, ctypes.POINTER(u32)]
    L.dcs_decode_batch.restype = i32
    L.dcs_decode_batch.argtypes = [vp, vp, sz, vp, u32, vp, u32, vp, u32, vp, vp, vp]
    L.dcs_batch_create.restype = i32
    L.dcs_batch_create.argtypes = [vp, vp, sz, vp, u32, vp, u32, vp, u32, ctypes.POINTER(vp)]
    if hasattr(L, "dcs_batch_create_mids"):             # (DCS_HIP_LIB may name a build from before the even deal: A/B against it)
        L.dcs_batch_create_mids.restype = i32
        L.dcs_batch_create_mids.argtypes = [vp, vp, sz, vp, vp, u32, vp, u32, vp, u32, ctypes.POINTER(vp)]
        L.dcs_index_stream_mids.restype = i32
        L.dcs_index_stream_mids.argtypes = [ctypes.c_int, vp, sz, vp, u32, ctypes.POINTER(StreamInfo), vp]
        L.dcs_index_streams_mids.restype = i32
        L.dcs_index_streams_mids.argtypes = [vp, u32, ctypes.c_int, vp, vp, vp, vp]
        L.dcs_ctx_set_even_deal.restype = i32
        L.dcs_ctx_set_even_deal.argtypes = [vp, ctypes.c_int]
        L.dcs_batch_even_deal.restype = ctypes.c_int
        L.dcs_batch_even_deal.argtypes = [vp]
        L.dcs_pack_chunks_mids.restype = i32
        L.dcs_pack_chunks_mids.argtypes = [vp, u32, vp, vp, vp, sz, ctypes.c_int, vp, sz, ctypes.POINTER(u32), ctypes.POINTER(u32)]
        L.dcs_even_deal_lane.restype = None
        L.dcs_even_deal_lane.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.POINTER(ctypes.c_int)] * 3
    if hasattr(L, "dcs_ctx_set_sole_source_kernel"):    # (DCS_HIP_LIB may name a build from before there were these kernels: A/B against it)
        L.dcs_ctx_set_sole_source_kernel.restype = i32
        L.dcs_ctx_set_sole_source_kernel.argtypes = [vp, ctypes.c_int]
        L.dcs_batch_sole_source_kernel.restype = ctypes.c_int
        L.dcs_batch_sole_source_kernel.argtypes = [vp]
    if hasattr(L, "dcs_batch_filled_bands"):            # (likewise: a build from before the short pre-pass)
        L.dcs_batch_filled_bands.restype = ctypes.c_int
        L.dcs_batch_filled_bands.argtypes = [vp]
        L.dcs_prepass_short.restype = ctypes.c_int
        L.dcs_prepass_short.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.dcs_batch_destroy.restype = None
    L.dcs_batch_destroy.argtypes = [vp]
    L.dcs_batch_run.restype = i32
    L.dcs_batch_run.argtypes = [vp, vp]
    L.dcs_batch_run_many.restype = i32
    L.dcs_batch_run_many.argtypes = [vp, vp, ctypes.c_int]
    L.dcs_batch_time.restype = i32
    L.dcs_batch_time.argtypes = [vp, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
    L.dcs_batch_time_rotating.restype = i32
    L.dcs_batch_time_rotating.argtypes = [ctypes.POINTER(vp), u32, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
    L.dcs_batch_sync.restype = i32
    L.dcs_batch_sync.argtypes = [vp]
    L.dcs_batch_download.restype = i32
    L.dcs_batch_download.argtypes = [vp, vp, vp, vp]
    L.dcs_batch_download_view.restype = i32
    L.dcs_batch_download_view.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.dcs_batch_device_pcm.restype = vp
    L.dcs_batch_device_pcm.argtypes = [vp]
    L.dcs_batch_algorithmic_bytes.restype = ctypes.c_uint64
    L.dcs_batch_algorithmic_bytes.argtypes = [vp]
    L.dcs_batch_num_jobs.restype = u32
    L.dcs_batch_num_jobs.argtypes = [vp]
    L.dcs_decode_streams.restype = i32
    L.dcs_decode_streams.argtypes = [vp, vp, u32, u32, vp, sz, vp, vp]
    L.dcs_count_stream_frames.restype = i32
    L.dcs_count_stream_frames.argtypes = [vp, u32, u32, ctypes.POINTER(ctypes.c_uint64)]
    L.dcs_synth_stream.restype = i32
    L.dcs_synth_stream.argtypes = [ctypes.POINTER(SynthParams), vp, sz, ctypes.POINTER(sz)]
    L.dcs_plan_chunks.restype = i32
    L.dcs_plan_chunks.argtypes = [vp, u32, vp, ctypes.c_int, vp, sz, ctypes.POINTER(u32)]
    L.dcs_stream_params_from.restype = i32
    L.dcs_stream_params_from.argtypes = [i32, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint16, u32, vp, vp]
    L.dcs_decode_stream_sequence.restype = i32
    L.dcs_decode_stream_sequence.argtypes = [vp, vp, u32, u32, vp, sz, vp, vp]
    L.dcs_wav_header.restype = None
    L.dcs_wav_header.argtypes = [u32, vp]
    L.dcs_dcsa_header.restype = i32
    L.dcs_dcsa_header.argtypes = [i32, u32, vp]
    L.dcs_dcsa_parse.restype = i32
    L.dcs_dcsa_parse.argtypes = [vp, sz, ctypes.POINTER(i32), ctypes.POINTER(vp), ctypes.POINTER(u32)]
    L.dcs_write_wav.restype = i32
    L.dcs_write_wav.argtypes = [ctypes.c_char_p, vp, u32]
    L.dcs_write_dcsa.restype = i32
    L.dcs_write_dcsa.argtypes = [ctypes.c_char_p, i32, vp, u32]
    L.dcs_frame_diff.restype = ctypes.c_int
    L.dcs_frame_diff.argtypes = [ctypes.c_uint64, vp, vp, ctypes.c_char_p, sz, ctypes.POINTER(sz)]
    L.dcs_romset_create.restype = vp
    L.dcs_romset_create.argtypes = []
    L.dcs_romset_destroy.restype = None
    L.dcs_romset_destroy.argtypes = [vp]
    L.dcs_romset_last_error.restype = ctypes.c_char_p
    L.dcs_romset_last_error.argtypes = [vp]
    L.dcs_romset_add_rom.restype = i32
    L.dcs_romset_add_rom.argtypes = [vp, ctypes.c_int, ctypes.c_char_p, sz]
    L.dcs_romset_load_zip.restype = i32
    L.dcs_romset_load_zip.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p]
    L.dcs_romset_load_zip_memory.restype = i32
    L.dcs_romset_load_zip_memory.argtypes = [vp, ctypes.c_char_p, sz, ctypes.c_char_p, ctypes.c_char_p]
    L.dcs_romset_check.restype = i32
    L.dcs_romset_check.argtypes = [vp, ctypes.POINTER(RomCheck)]
    L.dcs_romset_set_version.restype = i32
    L.dcs_romset_set_version.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    L.dcs_romset_num_tracks.restype = u32
    L.dcs_romset_num_tracks.argtypes = [vp]
    L.dcs_romset_pointer.restype = i32
    L.dcs_romset_pointer.argtypes = [vp, u32, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_int)]
    L.dcs_romset_track_info.restype = i32
    L.dcs_romset_track_info.argtypes = [vp, u32, ctypes.POINTER(TrackInfo)]
    L.dcs_romset_decompile.restype = i32
    L.dcs_romset_decompile.argtypes = [vp, u32, vp, u32, ctypes.POINTER(u32)]
    L.dcs_romset_list_streams.restype = i32
    L.dcs_romset_list_streams.argtypes = [vp, vp, u32, ctypes.POINTER(u32)]
    L.dcs_romset_extract_plan.restype = i32
    L.dcs_romset_extract_plan.argtypes = [vp, vp, u32, ctypes.POINTER(u32)]
    L.dcs_romset_extract_tracks_plan.restype = i32
    L.dcs_romset_extract_tracks_plan.argtypes = [vp, vp, u32, ctypes.POINTER(u32)]
    L.dcs_extract_tracks.restype = i32
    L.dcs_extract_tracks.argtypes = [vp, vp, vp, u32, vp, sz, vp, vp]
    L.dcs_romset_stream_refs.restype = i32
    L.dcs_romset_stream_refs.argtypes = [vp, vp, u32, ctypes.c_int, vp]
    L.dcs_seq_create.restype = vp
    L.dcs_seq_create.argtypes = [vp]
    L.dcs_seq_destroy.restype = None
    L.dcs_seq_destroy.argtypes = [vp]
    L.dcs_seq_last_error.restype = ctypes.c_char_p
    L.dcs_seq_last_error.argtypes = [vp]
    for name, args in (("dcs_seq_set_master_volume", [vp, ctypes.c_int]), ("dcs_seq_set_reported_version", [vp, ctypes.c_uint16]),
                       ("dcs_seq_write_data_port", [vp, ctypes.c_uint8]), ("dcs_seq_add_track_command", [vp, ctypes.c_uint16]),
                       ("dcs_seq_clear_tracks", [vp]), ("dcs_seq_load_audio_stream", [vp, ctypes.c_int, u32, ctypes.c_int]),
                       ("dcs_seq_plan", [vp, u32]), ("dcs_seq_decode", [vp, vp, vp, sz, vp])):
        getattr(L, name).restype = i32
        getattr(L, name).argtypes = args
    L.dcs_seq_create_standalone.restype = vp
    L.dcs_seq_create_standalone.argtypes = [i32]
    L.dcs_seq_load_audio_stream_mem.restype = i32
    L.dcs_seq_load_audio_stream_mem.argtypes = [vp, ctypes.c_int, ctypes.c_char_p, sz, ctypes.c_int]
    L.dcs_seq_rewind.restype = i32
    L.dcs_seq_rewind.argtypes = [vp, u32]
    L.dcs_seq_plan_ahead.restype = i32
    L.dcs_seq_plan_ahead.argtypes = [vp, u32, u32, ctypes.POINTER(u32)]
    L.dcs_seq_decode_view.restype = i32
    L.dcs_seq_decode_view.argtypes = [vp, vp, ctypes.POINTER(vp), ctypes.POINTER(u32), ctypes.POINTER(vp)]
    L.dcs_seq_stream_playing_at.restype = ctypes.c_int
    L.dcs_seq_stream_playing_at.argtypes = [vp, u32, ctypes.c_int]
    L.dcs_seq_stream_playing.restype = ctypes.c_int
    L.dcs_seq_stream_playing.argtypes = [vp, ctypes.c_int]
    L.dcs_seq_tracks_active_at.restype = ctypes.c_int
    L.dcs_seq_tracks_active_at.argtypes = [vp, u32]
    L.dcs_ctx_call_floor.restype = i32
    L.dcs_ctx_call_floor.argtypes = [vp, u32, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    L.dcs_decode_batch_live.restype = i32
    L.dcs_decode_batch_live.argtypes = [vp, vp, sz, ctypes.c_uint64, vp, u32, vp, u32, vp, u32, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.dcs_seq_set_rewindable.restype = i32
    L.dcs_seq_set_rewindable.argtypes = [vp, ctypes.c_int]
    L.dcs_seq_pending_ticks.restype = u32
    L.dcs_seq_pending_ticks.argtypes = [vp]
    L.dcs_seq_is_fatal.restype = ctypes.c_int
    L.dcs_seq_is_fatal.argtypes = [vp]
    L.dcs_seq_host_bytes.restype = u32
    L.dcs_seq_host_bytes.argtypes = [vp, vp, u32]
    L.dcs_index_streams.restype = i32
    L.dcs_index_streams.argtypes = [vp, u32, ctypes.c_int, vp, vp, vp]
    L.dcs_index_streams_gpu.restype = i32
    L.dcs_index_streams_gpu.argtypes = [vp, vp, sz, vp, u32, vp, ctypes.c_uint64, vp]
    L.dcs_index_streams_gpu_time.restype = i32
    L.dcs_index_streams_gpu_time.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
    L.dcs_pack_chunks_device.restype = i32
    L.dcs_pack_chunks_device.argtypes = [vp, vp, u32, vp, u32, vp, sz, ctypes.c_int, vp, sz, ctypes.POINTER(u32), ctypes.POINTER(u32)]
    L.dcs_ctx_set_frames_per_chunk.restype = i32
    L.dcs_ctx_set_frames_per_chunk.argtypes = [vp, ctypes.c_int]
    L.dcs_batch_abi_bytes.restype = ctypes.c_uint64
    L.dcs_batch_abi_bytes.argtypes = [vp]
    L.dcs_batch_num_chunks.restype = u32
    L.dcs_batch_num_chunks.argtypes = [vp]
    L.dcs_batch_package_bytes.restype = u32
    L.dcs_batch_package_bytes.argtypes = [vp]
    L.dcs_ctx_set_batch_tails.restype = i32
    L.dcs_ctx_set_batch_tails.argtypes = [vp, ctypes.c_int]
    L.dcs_runtime_defaults.restype = ctypes.c_int
    L.dcs_runtime_defaults.argtypes = []
    L.dcs_batch_frames_per_wave.restype = ctypes.c_int
    L.dcs_batch_frames_per_wave.argtypes = [vp]
    if hasattr(L, "dcs_batch_chunks_per_wave"):
        L.dcs_batch_chunks_per_wave.restype = ctypes.c_int
        L.dcs_batch_chunks_per_wave.argtypes = [vp]
    L.dcs_ctx_clock_mhz.restype = i32
    L.dcs_ctx_clock_mhz.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    L.dcs_ctx_link_rate.restype = i32
    L.dcs_ctx_link_rate.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    L.dcs_ctx_set_test_hooks.restype = i32
    L.dcs_ctx_set_test_hooks.argtypes = [vp, u32, ctypes.c_int]
    L.dcs_pipeline_create.restype = i32
    L.dcs_pipeline_create.argtypes = [vp, ctypes.c_int, u32, ctypes.POINTER(vp)]
    L.dcs_pipeline_destroy.restype = None
    L.dcs_pipeline_destroy.argtypes = [vp]
    L.dcs_pipeline_submit.restype = i32
    L.dcs_pipeline_submit.argtypes = [vp, vp, u32, u32]
    L.dcs_pipeline_collect.restype = i32
    L.dcs_pipeline_collect.argtypes = [vp, ctypes.POINTER(PipelineResult)]
    L.dcs_pipeline_collect_flac.restype = i32
    L.dcs_pipeline_collect_flac.argtypes = [vp, ctypes.POINTER(PipelineFlacResult)]
    L.dcs_device_path_create.restype = i32
    L.dcs_device_path_create.argtypes = [vp, vp, u32, u32, ctypes.POINTER(vp)]
    L.dcs_device_path_run.restype = i32
    L.dcs_device_path_run.argtypes = [vp, ctypes.c_int, ctypes.POINTER(DevicePathTimes)]
    L.dcs_device_path_run_many.restype = i32
    L.dcs_device_path_run_many.argtypes = [vp, ctypes.c_int]
    L.dcs_device_path_download.restype = i32
    L.dcs_device_path_download.argtypes = [vp, vp, vp, vp]
    L.dcs_device_path_destroy.restype = None
    L.dcs_device_path_destroy.argtypes = [vp]
    L.dcs_node_create.restype = i32
    L.dcs_node_create.argtypes = [vp, u32, ctypes.c_int, u32, ctypes.POINTER(vp)]
    L.dcs_node_destroy.restype = None
    L.dcs_node_destroy.argtypes = [vp]
    L.dcs_node_submit.restype = i32
    L.dcs_node_submit.argtypes = [vp, vp, u32, u32]
    L.dcs_node_collect.restype = i32
    L.dcs_node_collect.argtypes = [vp, ctypes.POINTER(PipelineResult), ctypes.POINTER(ctypes.c_int)]
    L.dcs_node_num_devices.restype = u32
    L.dcs_node_num_devices.argtypes = [vp]
    L.dcs_node_device_info.restype = i32
    L.dcs_node_device_info.argtypes = [vp, u32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint64)]
    L.dcs_node_last_error.restype = ctypes.c_char_p
    L.dcs_node_last_error.argtypes = [vp]
    L.dcs_node_cache_release.restype = None
    L.dcs_node_cache_release.argtypes = []
    L.dcs_encode_params_default.restype = i32
    L.dcs_encode_params_default.argtypes = [ctypes.POINTER(EncodeParams)]
    L.dcs_encode_bound.restype = sz
    L.dcs_encode_bound.argtypes = [ctypes.c_uint64]
    L.dcs_encode_header.restype = i32
    L.dcs_encode_header.argtypes = [vp, vp, vp, ctypes.POINTER(EncodeParams), i32, i32, vp, ctypes.POINTER(i32), vp]
    L.dcs_encode_streams.restype = i32
    L.dcs_encode_streams.argtypes = [vp, vp, vp, u32, ctypes.POINTER(EncodeParams), vp, sz, vp, vp]
    L.dcs_encode93_bound.restype = sz
    L.dcs_encode93_bound.argtypes = [ctypes.c_uint64]
    L.dcs_encode93_header.restype = i32
    L.dcs_encode93_header.argtypes = [vp, vp, vp, ctypes.POINTER(EncodeParams), i32, vp, ctypes.POINTER(i32), vp]
    L.dcs_encode93_streams.restype = i32
    L.dcs_encode93_streams.argtypes = [vp, vp, vp, u32, ctypes.POINTER(EncodeParams), vp, sz, vp, vp]
    L.dcs_encode93a_bound.restype = sz
    L.dcs_encode93a_bound.argtypes = [ctypes.c_uint64]
    L.dcs_encode93a_streams.restype = i32
    L.dcs_encode93a_streams.argtypes = [vp, vp, vp, u32, ctypes.POINTER(EncodeParams), vp, sz, vp, vp, vp]
    L.dcs_transcode_plan.restype = i32
    L.dcs_transcode_plan.argtypes = [vp, u32, ctypes.POINTER(EncodeParams), u32, vp, vp]
    L.dcs_transcode_streams.restype = i32
    L.dcs_transcode_streams.argtypes = [vp, vp, u32, ctypes.POINTER(EncodeParams), u32, vp, sz, vp, vp]
    L.dcs_resample_filter_default.restype = i32
    L.dcs_resample_filter_default.argtypes = [ctypes.POINTER(ResampleFilter)]
    L.dcs_resample_count.restype = i32
    L.dcs_resample_count.argtypes = [ctypes.c_uint64, u32, i32, ctypes.POINTER(ResampleFilter), u32, ctypes.POINTER(ctypes.c_uint64)]
    L.dcs_resample_streams.restype = i32
    L.dcs_resample_streams.argtypes = [vp, vp, vp, u32, vp, vp, ctypes.POINTER(ResampleFilter), u32, vp, sz, vp]
    L.dcs_encode_streams_at.restype = i32
    L.dcs_encode_streams_at.argtypes = [vp, vp, vp, u32, vp, vp, ctypes.POINTER(ResampleFilter), u32, ctypes.POINTER(EncodeParams),
                                        vp, sz, vp, vp]
    L.dcs_wav_parse.restype = i32
    L.dcs_wav_parse.argtypes = [vp, sz, ctypes.POINTER(WavInfo)]
    L.dcs_encode_sweep.restype = i32
    L.dcs_encode_sweep.argtypes = [vp, vp, vp, u32, vp, u32, vp, u32, u32, vp, vp, sz, vp]
    L.dcs_encode_rd_bound.restype = sz
    L.dcs_encode_rd_bound.argtypes = [ctypes.c_uint64]
    L.dcs_encode_rd_streams.restype = i32
    L.dcs_encode_rd_streams.argtypes = [vp, vp, vp, u32, ctypes.POINTER(EncodeParams), vp, vp, ctypes.c_uint64, vp, vp, vp]
    L.dcs_encode93_rd_bound.restype = sz
    L.dcs_encode93_rd_bound.argtypes = [ctypes.c_uint64]
    L.dcs_encode93_rd_streams.restype = i32
    L.dcs_encode93_rd_streams.argtypes = L.dcs_encode_rd_streams.argtypes
    if hasattr(L, "dcs_encode_rd_fit"):     # (DCS_HIP_LIB may name a build from before there was a shared budget: A/B against it)
        L.dcs_encode_rd_fit.restype = i32
        L.dcs_encode_rd_fit.argtypes = [vp, vp, vp, u32, ctypes.POINTER(EncodeParams), ctypes.c_uint64, vp, vp, ctypes.c_uint64, vp, vp, vp, vp]
        L.dcs_encode93_rd_fit.restype = i32
        L.dcs_encode93_rd_fit.argtypes = L.dcs_encode_rd_fit.argtypes
        L.dcs_encode_rd_allot.restype = i32
        L.dcs_encode_rd_allot.argtypes = [vp, vp, vp, vp, u32, ctypes.c_uint64, vp, vp, vp]
    if hasattr(L, "dcs_encode_files_budget"):   # (as above: a build from before the budget calls took other sources)
        L.dcs_encode_streams_at_budget.restype = i32
        L.dcs_encode_streams_at_budget.argtypes = [vp, vp, vp, u32, vp, vp, ctypes.POINTER(ResampleFilter), u32, ctypes.POINTER(EncodeParams),
                                                   ctypes.POINTER(Budget), vp, sz, vp, vp, vp, vp, u32, vp]
        L.dcs_transcode_plan_budget.restype = i32
        L.dcs_transcode_plan_budget.argtypes = [vp, u32, ctypes.POINTER(EncodeParams), u32, ctypes.POINTER(Budget), vp, vp]
        L.dcs_transcode_streams_budget.restype = i32
        L.dcs_transcode_streams_budget.argtypes = [vp, vp, u32, ctypes.POINTER(EncodeParams), u32, ctypes.POINTER(Budget), vp, sz, vp, vp, vp]
        L.dcs_encode_files_plan_budget.restype = i32
        L.dcs_encode_files_plan_budget.argtypes = [vp, vp, u32, ctypes.POINTER(EncodeParams), ctypes.POINTER(ResampleFilter), u32,
                                                   ctypes.POINTER(Budget), vp, vp]
        L.dcs_encode_files_budget.restype = i32
        L.dcs_encode_files_budget.argtypes = [vp, vp, vp, u32, ctypes.POINTER(EncodeParams), ctypes.POINTER(ResampleFilter), u32,
                                              ctypes.POINTER(Budget), vp, sz, vp, vp, vp, vp, u32, vp]
    L.dcs_encode93a_sweep.restype = i32
    L.dcs_encode93a_sweep.argtypes = [vp, vp, vp, u32, vp, u32, vp, u32, u32, vp, vp, vp, sz, vp]
    L.dcs_encode_sweep_group_frames.restype = None
    L.dcs_encode_sweep_group_frames.argtypes = [ctypes.c_uint64]
    L.dcs_encode_fit.restype = i32
    L.dcs_encode_fit.argtypes = [vp, vp, u32, u32, ctypes.c_uint64, vp, vp]
    L.dcs_encode_files_plan.restype = i32
    L.dcs_encode_files_plan.argtypes = [vp, vp, u32, ctypes.POINTER(EncodeParams), ctypes.POINTER(ResampleFilter), u32, vp, vp, vp]
    L.dcs_wav_decode.restype = i32
    L.dcs_wav_decode.argtypes = [vp, vp, vp, u32, vp, sz, vp]
    L.dcs_flac_parse.restype = i32
    L.dcs_flac_parse.argtypes = [vp, sz, ctypes.POINTER(FlacInfo)]
    L.dcs_flac_index.restype = i32
    L.dcs_flac_index.argtypes = [vp, sz, vp, u32, vp]
    L.dcs_flac_decode.restype = i32
    L.dcs_flac_decode.argtypes = [vp, vp, vp, u32, vp, sz, vp]
    L.dcs_flac_write_bound.restype = ctypes.c_uint64
    L.dcs_flac_write_bound.argtypes = [ctypes.c_uint64]
    L.dcs_flac_write_check.restype = i32
    L.dcs_flac_write_check.argtypes = [vp, u32, u32, u32, vp]
    L.dcs_flac_write_streams.restype = i32
    L.dcs_flac_write_streams.argtypes = [vp, vp, vp, u32, u32, u32, vp, sz, vp, vp]
    L.dcs_decode_streams_flac.restype = i32
    L.dcs_decode_streams_flac.argtypes = [vp, vp, u32, u32, u32, vp, sz, vp, vp, vp]
    L.dcs_encode_files.restype = i32
    L.dcs_encode_files.argtypes = [vp, vp, vp, u32, ctypes.POINTER(EncodeParams), ctypes.POINTER(ResampleFilter), u32, vp, sz,
                                   vp, vp]
    if hasattr(L, "dcs_decode_streams_at"):     # (DCS_HIP_LIB may name a build from before there was an output rate)
        L.dcs_resample_out_count.restype = i32
        L.dcs_resample_out_count.argtypes = [ctypes.c_uint64, u32, ctypes.POINTER(ResampleFilter), u32, ctypes.POINTER(ctypes.c_uint64)]
        L.dcs_resample_out_walk.restype = i32
        L.dcs_resample_out_walk.argtypes = [ctypes.c_uint64, u32, ctypes.POINTER(ResampleFilter), u32, vp, vp, ctypes.c_uint64,
                                            ctypes.POINTER(ctypes.c_uint64)]
        L.dcs_resample_out_streams.restype = i32
        L.dcs_resample_out_streams.argtypes = [vp, vp, vp, u32, u32, ctypes.POINTER(ResampleFilter), u32, vp, sz, vp, vp]
        L.dcs_decode_streams_at.restype = i32
        L.dcs_decode_streams_at.argtypes = [vp, vp, u32, u32, u32, ctypes.POINTER(ResampleFilter), u32, vp, sz, vp, vp, vp]
    if hasattr(L, "dcs_decode_streams_flac_at"):    # (... or from before the writer took streams of any length)
        L.dcs_flac_write_samples_check.restype = i32
        L.dcs_flac_write_samples_check.argtypes = [vp, u32, u32, u32, vp]
        L.dcs_flac_write_samples.restype = i32
        L.dcs_flac_write_samples.argtypes = [vp, vp, vp, u32, u32, u32, vp, sz, vp, vp]
        L.dcs_decode_streams_flac_at.restype = i32
        L.dcs_decode_streams_flac_at.argtypes = [vp, vp, u32, u32, u32, ctypes.POINTER(ResampleFilter), u32, vp, sz, vp, vp, vp, vp]
    if hasattr(L, "dcs_level_gain"):        # (DCS_HIP_LIB may name a build from before there was the level stage: A/B against it)
        fp = ctypes.POINTER(ctypes.c_float)
        L.dcs_level_gain.restype = i32
        L.dcs_level_gain.argtypes = [ctypes.c_float, ctypes.POINTER(Level), ctypes.c_float, fp, fp]
        L.dcs_level_streams.restype = i32
        L.dcs_level_streams.argtypes = [vp, vp, vp, u32, vp, u32, vp, sz, vp, vp]
        L.dcs_resample_streams_level.restype = i32
        L.dcs_resample_streams_level.argtypes = L.dcs_resample_streams.argtypes + [vp, u32, vp]
        L.dcs_encode_streams_at_level.restype = i32
        L.dcs_encode_streams_at_level.argtypes = L.dcs_encode_streams_at.argtypes + [vp, u32, vp]
        L.dcs_encode_files_level.restype = i32
        L.dcs_encode_files_level.argtypes = L.dcs_encode_files.argtypes + [vp, u32, vp]
    L.dcs_device_numa_node.restype = ctypes.c_int
    L.dcs_device_numa_node.argtypes = [ctypes.c_int]
    L.dcs_host_threads.restype = ctypes.c_int
    L.dcs_host_threads.argtypes = []
    L.dcs_partition_streams.restype = i32
    L.dcs_partition_streams.argtypes = [vp, u32, u32, vp]
    L.dcs_decode_streams_sharded.restype = i32
    L.dcs_decode_streams_sharded.argtypes = [vp, u32, vp, u32, u32, vp, sz, vp, vp, vp]
    _LIB = L
    return L


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _check(st, ctx=None):
    if st != 0:
        msg = load_library().dcs_last_error(ctx)
        raise DcsError(st, msg.decode() if msg else "")


# ---------------------------------------------------------------------------------------------- host side
def _index_one(entry, os_, stream, with_mids=False):
    """one stream through `entry` of the library: (records, StreamInfo), and the mid records where the entry makes them"""
    buf = np.frombuffer(bytes(stream), dtype=np.uint8)
    nframes = (int(buf[0]) << 8) | int(buf[1])
    out = np.zeros(max(nframes, 1), dtype=INDEX_DTYPE)
    mids = (np.zeros((max(nframes, 1), 16), dtype=np.uint32),) if with_mids else ()
    info = StreamInfo()
    st = entry(os_, _ptr(buf), buf.size, _ptr(out), nframes, ctypes.byref(info), *[_ptr(m) for m in mids])
    if st != 0:
        raise DcsError(st)
    return (out[:info.nValidFrames], info) + tuple(m[:info.nValidFrames] for m in mids)


def index_stream(os_, stream, literal=False):
    """dcs_index_stream (literal: dcs_index_stream_literal): returns (index records as INDEX_DTYPE array, StreamInfo)"""
    L = load_library()
    return _index_one(L.dcs_index_stream_literal if literal else L.dcs_index_stream, os_, stream)


class SrcArray(np.ndarray):
    """source descriptors with the mid records of their frames riding along (`mids`: MIDS_DTYPE [n, 16], or None), so that
    Context.batch(blob, srcs, jobs) can hand them on.  A slice or a copy is a plain array again: the records would no longer
    be parallel to it, and the batch keeps whole bands.  Rows edited in place are the caller's business as with any
    descriptor; mid records that no longer fit the index records are refused when the batch is made."""
    mids = None

    def __array_finalize__(self, obj):
        self.mids = None


def index_stream_mids(os_, stream):
    """dcs_index_stream_mids: (index records, StreamInfo, mid records [frames, 16] uint32) -- the middle of every 1994+ band of
    16 or 32 samples, for the even deal of dcs_batch_create_mids"""
    return _index_one(load_library().dcs_index_stream_mids, os_, stream, with_mids=True)


def _info_from_record(r):
    info = StreamInfo()
    ctypes.memmove(ctypes.byref(info), r.tobytes(), ctypes.sizeof(info))
    return info


def _frame_counts(streams):
    return np.array([(s[1][0] << 8) | s[1][1] for s in streams], dtype=np.uint64)


def _split_records(out, infos, first):
    return [(out[int(first[k]):int(first[k]) + int(infos[k]["nValidFrames"])], _info_from_record(infos[k]))
            for k in range(len(infos))]


def index_streams(streams, threads=0, with_mids=False):
    """dcs_index_streams: index many (os, bytes, ...) streams on `threads` host threads (0 = all).
    Returns a list of (records, StreamInfo), one per stream, identical to index_stream on each; with_mids
    (dcs_index_streams_mids): of (records, StreamInfo, mid records) as index_stream_mids returns them."""
    L = load_library()
    streams = list(streams)
    if not streams:
        return []
    counts = _frame_counts(streams)
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    keep = [np.frombuffer(bytes(s[1]), dtype=np.uint8) for s in streams]
    refs = (StreamRef * len(streams))()
    for k, s in enumerate(streams):
        refs[k].data = keep[k].ctypes.data
        refs[k].len = keep[k].size
        refs[k].os = s[0]
    out = np.zeros(max(int(first[-1]), 1), dtype=INDEX_DTYPE)
    infos = np.zeros(len(streams), dtype=INFO_DTYPE)
    mids = (np.zeros((out.size, 16), dtype=np.uint32),) if with_mids else ()
    entry = L.dcs_index_streams_mids if with_mids else L.dcs_index_streams
    st = entry(refs, len(streams), threads, _ptr(out), _ptr(first), _ptr(infos), *[_ptr(m) for m in mids])
    if st != 0:
        raise DcsError(st)
    return [(r, i) + tuple(m[int(first[k]):int(first[k]) + len(r)] for m in mids)
            for k, (r, i) in enumerate(_split_records(out, infos, first))]


def pack_streams(streams, pad=64):
    """Lay (os, bytes, ...) streams out in one dword-aligned blob: -> (blob bytes, LOC_DTYPE array)"""
    blob = bytearray()
    locs = np.zeros(len(streams), dtype=LOC_DTYPE)
    rec = 0
    for k, s in enumerate(streams):
        while len(blob) & 3:
            blob.append(0)
        data = bytes(s[1])
        locs[k] = (len(blob), len(data), s[0], rec)
        rec += (data[0] << 8) | data[1]
        blob += data
        blob += bytes(pad)
    return bytes(blob), locs


def volume_multiplier(vol):
    return load_library().dcs_volume_multiplier(vol)


def mixing_multiplier(os_, level_sum, channel_volume=0xFF):
    return load_library().dcs_mixing_multiplier(os_, level_sum, channel_volume)


def frame_scale(vol_mult, mix_muls, active=None):
    mm = np.ascontiguousarray(mix_muls, dtype=np.uint16).copy()
    act = None if active is None else np.ascontiguousarray(active, dtype=np.uint8)
    vs = load_library().dcs_frame_scale(vol_mult, _ptr(mm), _ptr(act), mm.size)
    return vs, mm


def stream_params(os_, volume, level, nframes, channel_volume=0xFF):
    mm = np.zeros(nframes, dtype=np.uint16)
    vs = np.zeros(nframes, dtype=np.uint8)
    _check(load_library().dcs_stream_params(os_, volume, level, channel_volume, nframes, _ptr(mm), _ptr(vs)))
    return mm, vs


def wav_header(nframes):
    out = np.zeros(44, dtype=np.uint8)
    load_library().dcs_wav_header(nframes, _ptr(out))
    return out.tobytes()


def dcsa_header(os_, nbytes):
    out = np.zeros(36, dtype=np.uint8)
    st = load_library().dcs_dcsa_header(os_, nbytes, _ptr(out))
    if st != 0:
        raise DcsError(st)
    return out.tobytes()


def dcsa_parse(data):
    """-> (os, stream bytes) of a "DCSa" container; raises DcsError(ERR_BAD_STREAM) if it is not one"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
    os_, ptr, n = ctypes.c_int32(), ctypes.c_void_p(), ctypes.c_uint32()
    st = load_library().dcs_dcsa_parse(_ptr(buf), len(data), ctypes.byref(os_), ctypes.byref(ptr), ctypes.byref(n))
    if st != 0:
        raise DcsError(st)
    off = ptr.value - buf.ctypes.data
    return os_.value, bytes(data)[off:off + n.value]


def frame_diff(frame_no, mine, theirs):
    """-> (number of differing samples, the block the reference's --validate log would hold)"""
    a = np.ascontiguousarray(mine, dtype=np.int16)
    b = np.ascontiguousarray(theirs, dtype=np.int16)
    assert a.size == FRAME_SAMPLES and b.size == FRAME_SAMPLES
    text = ctypes.create_string_buffer(8192)
    n = ctypes.c_size_t()
    d = load_library().dcs_frame_diff(frame_no, _ptr(a), _ptr(b), text, len(text), ctypes.byref(n))
    return d, text.raw[:n.value].decode()


def synth_stream(fmt, nframes, seed, nbands=16, stride_from=16, profile=0):
    L = load_library()
    p = SynthParams(seed=seed, format=fmt, nFrames=nframes, nBands=nbands, strideFromBand=stride_from,
                    profile=profile, reserved=0)
    n = ctypes.c_size_t(0)
    _check(L.dcs_synth_stream(ctypes.byref(p), None, 0, ctypes.byref(n)))
    out = np.zeros(n.value, dtype=np.uint8)
    _check(L.dcs_synth_stream(ctypes.byref(p), _ptr(out), out.size, ctypes.byref(n)))
    return out.tobytes()


def encode_params(fmt=None, **params):
    """an EncodeParams: the reference's defaults (dcs_encode_params_default), the layout `fmt` (None = wildcard,
    FMT_94_T0, FMT_94_T1_S0, FMT_94_T1_S3 or FMT_94_T0_S3) and any CompressionParams field by name"""
    p = EncodeParams()
    _check(load_library().dcs_encode_params_default(ctypes.byref(p)))
    if fmt not in _ENCODE_FMT:
        raise ValueError("no 1994+ encoder layout %r" % (fmt,))
    p.streamFormatType, p.streamFormatSubType = _ENCODE_FMT[fmt]
    for k, v in params.items():
        if k not in dict(EncodeParams._fields_) or k == "reserved":
            raise TypeError("unknown encoder parameter %r" % k)
        setattr(p, k, v)
    return p


def encode_bound(n_samples):
    """dcs_encode_bound: the largest stream n_samples samples can encode to (0 = not encodable)"""
    return int(load_library().dcs_encode_bound(int(n_samples)))


def encode_header(power_sum, lo, hi, fmt_type, fmt_sub_type, **params):
    """dcs_encode_header -> (16 header bytes, bandsToKeep, bitsPerBand[16])"""
    a = [np.ascontiguousarray(x, dtype=np.float32) for x in (power_sum, lo, hi)]
    assert all(x.shape == (16,) for x in a)
    p = encode_params(**params)
    hdr, bits, keep = np.zeros(16, np.uint8), np.zeros(16, np.int32), ctypes.c_int32()
    _check(load_library().dcs_encode_header(_ptr(a[0]), _ptr(a[1]), _ptr(a[2]), ctypes.byref(p), int(fmt_type), int(fmt_sub_type),
                                            _ptr(hdr), ctypes.byref(keep), _ptr(bits)))
    return hdr, keep.value, bits


# OS93: the format version per OS, and the layouts encode93_streams can be asked for (streamFormatType; None = wildcard)
_ENCODE93_VERSION = {OS93A: 0x9301, OS93B: 0x9302}
_ENCODE93_FMT = {None: -1, FMT_93_T0: 0, FMT_93B_T1: 1, FMT_93A_T1: 1}


def encode93_params(os_=OS93B, fmt=None, **params):
    """an EncodeParams for the OS93 encoder: the reference's defaults, formatVersion 0x9301 (OS93A) or 0x9302 (OS93B), the
    layout `fmt` (None = wildcard, FMT_93_T0, FMT_93B_T1 with OS93B, FMT_93A_T1 with OS93A) and CompressionParams by name"""
    if os_ not in _ENCODE93_VERSION:
        raise ValueError("no OS93 encoder for OS %r" % (os_,))
    if fmt not in _ENCODE93_FMT or (fmt == FMT_93B_T1 and os_ != OS93B) or (fmt == FMT_93A_T1 and os_ != OS93A):
        raise ValueError("no OS93 layout %r for OS %r" % (fmt, os_))
    return encode_params(None, **dict(dict(formatVersion=_ENCODE93_VERSION[os_], streamFormatType=_ENCODE93_FMT[fmt],
                                           streamFormatSubType=-1), **params))


def encode93_bound(n_samples):
    """dcs_encode93_bound: the largest OS93 stream n_samples samples can encode to (0 = not encodable)"""
    return int(load_library().dcs_encode93_bound(int(n_samples)))


# DcsEncode93aInfo: the Type-1 candidate of a stream encoded by encode93a_streams
ENCODE93A_INFO_DTYPE = np.dtype([("selector", "<i4"), ("ladderIndex", "<i4"), ("numBands", "<i4"), ("reserved", "<i4"),
                                 ("frameBits", "<u8"), ("budgetBits", "<u8"), ("sqErr", "<u8")])


def encode93a_bound(n_samples):
    """dcs_encode93a_bound: the largest stream n_samples samples can encode to through encode93a_streams, either type"""
    return int(load_library().dcs_encode93a_bound(int(n_samples)))


# DcsEncodeRdInfo: what the rate-distortion search of encode_rd_streams chose for a stream
ENCODE_RD_INFO_DTYPE = np.dtype([("formatType", "<i4"), ("formatSubType", "<i4"), ("ladderIndex", "<i4"), ("numBands", "<i4"),
                                 ("frameBits", "<u8"), ("budgetBits", "<u8"), ("sqErr", "<u8"), ("fits", "<i4"), ("reserved", "<i4")])


def encode_rd_bound(n_samples):
    """dcs_encode_rd_bound: the largest stream n_samples samples can encode to through encode_rd_streams (0 = not encodable)"""
    return int(load_library().dcs_encode_rd_bound(int(n_samples)))


def encode93_rd_bound(n_samples):
    """dcs_encode93_rd_bound: the largest stream n_samples samples can encode to through encode93_rd_streams (0 = not encodable)"""
    return int(load_library().dcs_encode93_rd_bound(int(n_samples)))


# DcsEncodeRdFitInfo: the allocator's record of encode_rd_fit, encode93_rd_fit and encode_rd_allot
ENCODE_RD_FIT_INFO_DTYPE = np.dtype([("totalBytes", "<u8"), ("leastBytes", "<u8"), ("usedBytes", "<u8"), ("sqErr", "<u8"),
                                     ("nSteps", "<u4"), ("stepsTaken", "<u4"), ("fits", "<i4"), ("reserved", "<i4")])


def encode_rd_allot(curves, total, caps=None, ctx=None):
    """dcs_encode_rd_allot: the allocator of DESIGN.md 10.13 alone.  curves: per job a sequence of (size in bytes, squared
    error) candidates; total: the bytes all jobs share; caps: per job the most bytes it may take (None: no caps).  ctx None:
    on the host; a Context: on its device.  Returns (allotments uint32 [jobs], ENCODE_RD_FIT_INFO_DTYPE record)."""
    n = len(curves)
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum([len(c) for c in curves], dtype=np.uint64)
    flat = [p for c in curves for p in c]
    size = np.array([int(p[0]) for p in flat], np.uint64)
    err = np.array([int(p[1]) for p in flat], np.uint64)
    cap = None if caps is None else np.ascontiguousarray(np.asarray(caps, np.int64).clip(0, 0xFFFFFFFF), dtype=np.uint32)
    if cap is not None and cap.shape != (n,):
        raise ValueError("encode_rd_allot: one cap per job")
    allot, fit = np.zeros(n, np.uint32), np.zeros(1, ENCODE_RD_FIT_INFO_DTYPE)
    L = load_library()
    st = L.dcs_encode_rd_allot(ctx.h if ctx is not None else None, _ptr(size) if len(flat) else None, _ptr(err) if len(flat) else None,
                               _ptr(offs), n, int(total), _ptr(cap) if cap is not None and n else None, _ptr(allot) if n else None, _ptr(fit))
    if ctx is not None:
        _check(st, ctx.h)
    elif st != 0:
        raise DcsError(st, "dcs_encode_rd_allot")
    return allot, fit[0]


def encode93a_params(fmt, **params):
    """the EncodeParams of an OS93a set (formatVersion 0x9301) for encode93a_sweep / encode93a_fit: fmt FMT_93A_T1 or
    FMT_93_T0 (None, the wildcard, is encode93a_streams' alone: a sweep refuses it), CompressionParams by name"""
    if fmt not in (None, FMT_93_T0, FMT_93A_T1):
        raise ValueError("no OS93a layout %r" % (fmt,))
    return encode_params(None, **dict(dict(formatVersion=0x9301, streamFormatType=_ENCODE93_FMT[fmt], streamFormatSubType=-1), **params))


def encode93_header(power_sum, lo, hi, fmt_type, os_=OS93B, **params):
    """dcs_encode93_header -> (16 header bytes, bandsToKeep, bitsPerBand[16])"""
    a = [np.ascontiguousarray(x, dtype=np.float32) for x in (power_sum, lo, hi)]
    assert all(x.shape == (16,) for x in a)
    p = encode93_params(os_, **params)
    hdr, bits, keep = np.zeros(16, np.uint8), np.zeros(16, np.int32), ctypes.c_int32()
    _check(load_library().dcs_encode93_header(_ptr(a[0]), _ptr(a[1]), _ptr(a[2]), ctypes.byref(p), int(fmt_type), _ptr(hdr),
                                              ctypes.byref(keep), _ptr(bits)))
    return hdr, keep.value, bits


def transcode_params(version=0x9400, fmt=None, **params):
    """the EncodeParams of a transcode target: formatVersion 0x9400 (fmt as encode_params) or 0x9301 / 0x9302 (fmt as
    encode93_params), CompressionParams by name"""
    if version == 0x9400:
        return encode_params(fmt, **params)
    if version in (0x9301, 0x9302):
        return encode93_params(TRANSCODE_OS[version], fmt, **params)
    raise ValueError("no encoder for formatVersion %#x" % version)


def _transcode_refs(streams, os_list, volume, level, channel_volume):
    streams = [bytes(s) for s in streams]
    os_list = list(os_list)
    if len(os_list) != len(streams):
        raise ValueError("%d streams, %d OS versions" % (len(streams), len(os_list)))
    keep = [np.frombuffer(s, dtype=np.uint8) if s else np.zeros(1, np.uint8) for s in streams]
    refs = (StreamRef * max(1, len(streams)))()
    for k, s in enumerate(streams):
        refs[k].data = keep[k].ctypes.data
        refs[k].len = len(s)
        refs[k].os = os_list[k]
        refs[k].volume = volume
        refs[k].level = level
        refs[k].channelVolume = channel_volume
    return refs, keep


def transcode_plan(streams, os_list, version=0x9400, fmt=None, reencode_all=False, volume=0x67, level=0xFF, channel_volume=0xFF,
                   **params):
    """dcs_transcode_plan (host only): -> (action per stream, TRANSCODE_COPIED / _REENCODED; the bytes its output can take)"""
    p = transcode_params(version, fmt, **params)
    refs, keep = _transcode_refs(streams, os_list, volume, level, channel_volume)
    n = len(keep) if streams else 0
    action, bound = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint64)
    _check(load_library().dcs_transcode_plan(refs, n, ctypes.byref(p), TRANSCODE_REENCODE_ALL if reencode_all else 0,
                                             _ptr(action), _ptr(bound)))
    return action[:n], bound[:n]


def _budget(n, budget, total, cap):
    """the DcsBudget of n jobs: budget None, an int or a sequence = per job; total not None = the shared form, with cap None,
    an int or a sequence.  -> (Budget, the ENCODE_RD_FIT_INFO_DTYPE array of one record it points to, what it keeps alive)"""
    def per_job(v):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.int64), (n,)).clip(0, 0xFFFFFFFF), dtype=np.uint32)
    b = Budget()
    fit = np.zeros(1, ENCODE_RD_FIT_INFO_DTYPE)
    bud = per_job(budget) if budget is not None and n else None
    caps = per_job(cap) if cap is not None and n else None
    b.budgetBytes = bud.ctypes.data if bud is not None else None
    b.capBytes = caps.ctypes.data if caps is not None else None
    b.shared = 0 if total is None else 1
    b.totalBytes = 0 if total is None else int(total)
    b.fit = fit.ctypes.data
    return b, fit, (bud, caps)


def transcode_plan_budget(streams, os_list, version=0x9400, fmt=None, reencode_all=False, budget=None, total=None, cap=None,
                          volume=0x67, level=0xFF, channel_volume=0xFF, **params):
    """dcs_transcode_plan_budget (host only): transcode_plan under the copy rule of transcode_streams_budget -> (action per
    stream, the bytes its output can take)"""
    p = transcode_params(version, fmt, **params)
    refs, keep = _transcode_refs(streams, os_list, volume, level, channel_volume)
    n = len(keep) if streams else 0
    b, _, alive = _budget(n, budget, total, cap)
    action, bound = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint64)
    _check(load_library().dcs_transcode_plan_budget(refs, n, ctypes.byref(p), TRANSCODE_REENCODE_ALL if reencode_all else 0,
                                                    ctypes.byref(b), _ptr(action), _ptr(bound)))
    del alive
    return action[:n], bound[:n]


def sweep_sq_err(results):
    """the squared error at unity of measured SWEEP_RESULT_DTYPE records, sumDecSq - 2 sumCross + sumSrcSq (Python ints)"""
    return [int(r["sumDecSq"]) - 2 * int(r["sumCross"]) + int(r["sumSrcSq"]) for r in np.atleast_1d(results)]


def encode_sweep_group_frames(max_job_frames):
    """dcs_encode_sweep_group_frames: the most job-frames a group of an encode may hold (0: what the memory takes)"""
    load_library().dcs_encode_sweep_group_frames(int(max_job_frames))


def encode_fit_choose(n_bytes, sq_err, budget):
    """dcs_encode_fit (host only): tables [nStreams][nSets], the sets in order of preference -> (choice per stream, total
    bytes).  Raises DcsError with status -5 when no set fits as a whole; its `needed` is the smallest column total and its
    `choice` that column."""
    nb = np.ascontiguousarray(n_bytes, dtype=np.uint64)
    se = np.ascontiguousarray(sq_err, dtype=np.uint64)
    if nb.ndim != 2 or nb.shape != se.shape:
        raise ValueError("n_bytes and sq_err are [nStreams][nSets] tables of one shape")
    choice = np.zeros(max(nb.shape[0], 1), np.int32)
    total = ctypes.c_uint64(0)
    st = load_library().dcs_encode_fit(_ptr(nb) if nb.size else None, _ptr(se) if se.size else None, nb.shape[0], nb.shape[1],
                                       int(budget), _ptr(choice), ctypes.byref(total))
    if st == -5:
        e = DcsError(st, "no parameter set fits %d bytes: the smallest needs %d" % (int(budget), total.value))
        e.needed = int(total.value)
        e.choice = choice[:nb.shape[0]].copy()
        raise e
    _check(st)
    return choice[:nb.shape[0]].copy(), int(total.value)


def _encode_input(pcm_list):
    parts = []
    for x in pcm_list:
        x = np.asarray(x)
        parts.append(x.astype(np.float32) / np.float32(32768.0) if x.dtype == np.int16 else np.asarray(x, dtype=np.float32))
    offs = np.zeros(len(parts) + 1, np.uint64)
    offs[1:] = np.cumsum([len(x) for x in parts])
    return (np.concatenate(parts) if parts else np.zeros(1, np.float32)), offs


def resample_filter_default():
    """dcs_resample_filter_default -> (float32 coefficients, increment): the library's own Kaiser-windowed sinc table"""
    f = ResampleFilter()
    _check(load_library().dcs_resample_filter_default(ctypes.byref(f)))
    c = np.ctypeslib.as_array(ctypes.cast(f.coeffs, ctypes.POINTER(ctypes.c_float)), shape=(f.nCoeffs,)).copy()
    return c, int(f.increment)


def _resample_filter(filter):
    """(ResampleFilter or None, the array it points into): filter = None (the default table) or (coefficients, increment)"""
    if filter is None:
        return None, None
    coeffs, increment = filter
    c = np.ascontiguousarray(coeffs, dtype=np.float32)
    return ResampleFilter(c.ctypes.data, len(c), int(increment)), c


def _per_stream(v, n, dtype, name):
    a = np.full(n, v, dtype) if np.ndim(v) == 0 else np.ascontiguousarray(v, dtype=dtype)
    if len(a) != n:
        raise ValueError("%d streams, %d %s" % (n, len(a), name))
    return a if n else np.zeros(1, dtype)


def _resample_bound(n_values, rate, channels, at_unity):
    """at least the resampled length of a stream (host arithmetic, no walk): its mono samples x 31250 / rate and a margin,
    which the end rule keeps the position chain inside"""
    m = (n_values + 1) // 2 if channels == 2 else n_values
    if rate == 31250 and not at_unity:
        return m
    return m * 31250 // max(rate, 1) + m // (1 << 20) + 8


def resample_count(n_values, rate, channels=1, filter=None, at_unity=False):
    """dcs_resample_count (host only): the number of 31 250 Hz samples n_values input values (interleaved when
    channels == 2) at `rate` Hz resample to; filter as Context.resample_streams"""
    f, keep = _resample_filter(filter)
    out = ctypes.c_uint64()
    _check(load_library().dcs_resample_count(int(n_values), int(rate), int(channels), ctypes.byref(f) if f is not None else None,
                                             RESAMPLE_AT_UNITY if at_unity else 0, ctypes.byref(out)))
    del keep
    return int(out.value)


def _resample_out_bound(n_samples, rate, at_unity):
    """at least the converted length of n_samples samples at 31 250 Hz (host arithmetic, no walk): the end rule keeps the
    position chain inside n_samples x rate / 31250, and the margin covers its rounding (INTEGRATION.md rule 40; the library's own
    bound on a walk, rsSlots, is n_samples x ratio + 4)"""
    if rate == 31250 and not at_unity:
        return n_samples
    return n_samples * max(rate, 0) // 31250 + 8


def resample_out_count(n_samples, rate, filter=None, at_unity=False):
    """dcs_resample_out_count (host only): the number of samples at `rate` Hz (4 000 .. 65 535) that n_samples samples at
    31 250 Hz convert to; filter as Context.resample_streams"""
    f, keep = _resample_filter(filter)
    out = ctypes.c_uint64()
    _check(load_library().dcs_resample_out_count(int(n_samples), int(rate), ctypes.byref(f) if f is not None else None,
                                                 RESAMPLE_AT_UNITY if at_unity else 0, ctypes.byref(out)))
    del keep
    return int(out.value)


def resample_out_walk(n_samples, rate, filter=None, at_unity=False):
    """dcs_resample_out_walk (host only, a diagnostic): the converter's walk of such a stream -> (int64 input positions,
    int32 start_filter_index values), one pair per output"""
    f, keep = _resample_filter(filter)
    fp = ctypes.byref(f) if f is not None else None
    flags = RESAMPLE_AT_UNITY if at_unity else 0
    cap = _resample_out_bound(int(n_samples), int(rate), at_unity)
    pos, sfi = np.zeros(max(cap, 1), np.int64), np.zeros(max(cap, 1), np.int32)
    count = ctypes.c_uint64()
    _check(load_library().dcs_resample_out_walk(int(n_samples), int(rate), fp, flags, _ptr(pos), _ptr(sfi), cap, ctypes.byref(count)))
    del keep
    if count.value > cap:
        raise DcsError(-1, "the walk made %d outputs, more than its bound %d" % (count.value, cap))
    return pos[:count.value].copy(), sfi[:count.value].copy()


def _levels(level, n):
    """level: a Level, or a list of n of them -> (DcsLevel array, its length)"""
    ls = [level] if isinstance(level, Level) else list(level)
    if len(ls) != 1 and len(ls) != n:
        raise ValueError("%d streams, %d levels (one, or one per stream)" % (n, len(ls)))
    return (Level * max(len(ls), 1))(*ls), len(ls)


def level_gain(peak, level, bound=1.0):
    """dcs_level_gain (host only): the gain `level` gives a stream whose peak is `peak`, and the peak after it, as float32.
    Raises DcsError -1 for a bad level, peak or bound, and -6 (with .gain and .peak_out) when the peak comes out above bound."""
    g, p = ctypes.c_float(), ctypes.c_float()
    st = load_library().dcs_level_gain(float(peak), ctypes.byref(level), float(bound), ctypes.byref(g), ctypes.byref(p))
    if st != 0:
        e = DcsError(st)
        if st == ERR_BAD_STREAM:
            e.gain, e.peak_out = np.float32(g.value), np.float32(p.value)
        raise e
    return np.float32(g.value), np.float32(p.value)


def _files_blob(files):
    """files (bytes, or paths) -> (uint8 blob, uint64 offsets)"""
    parts = []
    for f in files:
        if isinstance(f, (str, os.PathLike)):
            with open(f, "rb") as fh:
                f = fh.read()
        parts.append(np.frombuffer(bytes(f), dtype=np.uint8))
    offs = np.zeros(len(parts) + 1, np.uint64)
    offs[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
    blob = np.concatenate(parts) if parts and offs[-1] else np.zeros(1, np.uint8)
    return blob, offs


def wav_parse(data):
    """dcs_wav_parse (host only): one WAV file as libnyquist's WavDecoder reads it -> dict of the WavInfo fields (status 0 =
    accepted; otherwise the DcsStatus and `reason`)"""
    b = bytes(data)
    buf = np.frombuffer(b, dtype=np.uint8) if b else np.zeros(1, np.uint8)
    w = WavInfo()
    load_library().dcs_wav_parse(_ptr(buf), len(b), ctypes.byref(w))
    d = {k: getattr(w, k) for k, _ in WavInfo._fields_ if k != "reserved"}
    d["reason"] = w.reason.decode()
    return d


def flac_parse(data):
    """dcs_flac_parse (host only): one FLAC file's STREAMINFO and frame count as libFLAC reads them -> dict of the FlacInfo
    fields (status 0 = accepted; otherwise the DcsStatus and `reason`)"""
    b = bytes(data)
    buf = np.frombuffer(b, dtype=np.uint8) if b else np.zeros(1, np.uint8)
    w = FlacInfo()
    load_library().dcs_flac_parse(_ptr(buf), len(b), ctypes.byref(w))
    d = {k: getattr(w, k) for k, _ in FlacInfo._fields_}
    d["reason"] = w.reason.decode()
    return d


def flac_index(data):
    """dcs_flac_index (host only): -> (DcsStatus, FLAC_FRAME_DTYPE array of the file's frames; empty when refused)"""
    b = bytes(data)
    buf = np.frombuffer(b, dtype=np.uint8) if b else np.zeros(1, np.uint8)
    n = np.zeros(1, np.uint32)
    L = load_library()
    st = L.dcs_flac_index(_ptr(buf), len(b), None, 0, _ptr(n))
    if st != ERR_CAPACITY:
        return st, np.zeros(0, FLAC_FRAME_DTYPE)
    frames = np.zeros(int(n[0]), FLAC_FRAME_DTYPE)
    st = L.dcs_flac_index(_ptr(buf), len(b), _ptr(frames), frames.size, _ptr(n))
    return st, frames


def flac_write_bound(n_samples):
    """dcs_flac_write_bound: the largest FLAC stream n_samples samples can be written to"""
    return int(load_library().dcs_flac_write_bound(int(n_samples)))


def flac_write_check(lengths, rate=31250, flags=0):
    """dcs_flac_write_check on streams of `lengths` samples -> (status, the stream at fault)"""
    offs = np.concatenate(([0], np.cumsum(np.asarray(lengths, np.uint64)))).astype(np.uint64)
    bad = ctypes.c_uint32()
    st = load_library().dcs_flac_write_check(_ptr(offs), offs.size - 1, int(rate) & 0xFFFFFFFF, flags, ctypes.byref(bad))
    return st, bad.value


def flac_write_samples_check(lengths, rate, flags=0):
    """dcs_flac_write_samples_check on streams of `lengths` samples, any length from 1 on -> (status, the stream at fault)"""
    offs = np.concatenate(([0], np.cumsum(np.asarray(lengths, np.uint64)))).astype(np.uint64)
    bad = ctypes.c_uint32()
    st = load_library().dcs_flac_write_samples_check(_ptr(offs), offs.size - 1, int(rate) & 0xFFFFFFFF, flags, ctypes.byref(bad))
    return st, bad.value


def encode_files_plan(files, version=0x9400, fmt=None, filter=None, at_unity=False, **params):
    """dcs_encode_files_plan (host only): -> (kind per file, FILE_* or -1; the bytes its output can take; DcsStatus per file)"""
    p = transcode_params(version, fmt, **params)
    blob, offs = _files_blob(files)
    n = len(offs) - 1
    f, keep = _resample_filter(filter)
    kind, bound, status = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.int32)
    load_library().dcs_encode_files_plan(_ptr(blob), _ptr(offs), n, ctypes.byref(p), ctypes.byref(f) if f is not None else None,
                                         RESAMPLE_AT_UNITY if at_unity else 0, _ptr(kind), _ptr(bound), _ptr(status))
    del keep
    return kind[:n], bound[:n], status[:n]


def format_os(fmt, prefer_95=False, prefer_93a=False):
    """an OS version whose decoder parses `fmt`"""
    if fmt == FMT_93A_T1:
        return OS93A
    if fmt == FMT_93B_T1:
        return OS93B
    if fmt == FMT_93_T0:
        return OS93A if prefer_93a else OS93B
    return OS95 if prefer_95 else OS94


def build_stream_batch(streams, extra_frames=0, pad=64, indexer=None):
    """Host-side batch description for independent streams, each played alone from a fresh decoder
    (LoadAudioStream(0, ptr, level), DCSDecoderNative.cpp:1387).

    streams: iterable of (os, bytes, volume, level).  indexer: None (dcs_index_stream per stream), or a
    callable streams -> [(records, StreamInfo)] such as index_streams or Context.index_streams_gpu.
    Returns dict(blob, srcs, jobs, first_job)."""
    blob = bytearray()
    srcs, jobs, first, mids = [], [], [], []
    njobs = 0
    streams = list(streams)
    # (the host indexers also record the middles of the 1994+ bands: they ride along with the descriptors, see SrcArray)
    with_mids = (indexer is None or indexer is index_streams) and hasattr(load_library(), "dcs_index_stream_mids")
    if indexer is index_streams and with_mids:
        indexed = index_streams(streams, with_mids=True)
    else:
        indexed = indexer(streams) if indexer is not None else None
    for k, (os_, data, volume, level) in enumerate(streams):
        if with_mids:
            idx, info, m = indexed[k] if indexed is not None else index_stream_mids(os_, data)
            mids.append(m)
        else:
            idx, info = indexed[k] if indexed is not None else index_stream(os_, data)
        nframes = info.nFrames
        mm, vs = stream_params(os_, volume, level, nframes)
        while len(blob) & 3:
            blob.append(0)
        off = len(blob)
        blob += bytes(data)
        blob += bytes(max(pad, info.nBytes - len(data) + 8))     # bytes past a (damaged) stream's end read as zero
        nvalid = info.nValidFrames
        s = np.zeros(nvalid, dtype=SRC_DTYPE)
        s["streamOff"] = off
        s["mixMul"] = mm[:nvalid]
        s["format"] = info.format
        s["hdrLen"] = info.hdrLen
        s["idx"] = idx
        total = nframes + extra_frames
        j = np.zeros(total, dtype=JOB_DTYPE)
        nsrc_before = sum(len(x) for x in srcs)
        j["firstSrc"][:nvalid] = nsrc_before + np.arange(nvalid)
        j["nSrc"][:nvalid] = 1
        j["volShift"][:nvalid] = vs[:nvalid]
        j["volShift"][nvalid:] = 8
        j["xform"] = XFORM_93 if os_ in (OS93A, OS93B) else XFORM_94
        j["prev"] = njobs + np.arange(total, dtype=np.int64) - 1
        j["prev"][0] = PREV_NONE
        srcs.append(s)
        jobs.append(j)
        first.append(njobs)
        njobs += total
    first.append(njobs)
    all_srcs = (np.concatenate(srcs) if srcs else np.zeros(0, SRC_DTYPE)).view(SrcArray)
    if with_mids and mids:
        all_srcs.mids = np.ascontiguousarray(np.concatenate(mids), dtype=np.uint32)
    # (`mids` is the explicit form -- Context.batch(blob, srcs, jobs, mids=b["mids"]) --; the attribute on `srcs` serves callers
    # that hand on the three arrays only.  Either way dcs_batch_create_mids refuses mids that do not fit the records.)
    return dict(blob=bytes(blob), srcs=all_srcs, jobs=np.concatenate(jobs), first_job=np.array(first, dtype=np.int64),
                mids=all_srcs.mids)


def plan_chunks(jobs, fpw, srcs=None, handoff=True):
    """dcs_plan_chunks2 -> slots [nChunks, fpw] as a structured array (job, prevSlot, flags)"""
    L = load_library()
    jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
    srcs = None if srcs is None else np.ascontiguousarray(srcs, dtype=SRC_DTYPE)
    n = ctypes.c_uint32(0)
    _check(L.dcs_plan_chunks2(_ptr(jobs), jobs.size, _ptr(srcs), fpw, int(handoff), None, 0, ctypes.byref(n)))
    raw = np.zeros(n.value * fpw, dtype=np.uint64)
    _check(L.dcs_plan_chunks2(_ptr(jobs), jobs.size, _ptr(srcs), fpw, int(handoff), _ptr(raw), raw.size, ctypes.byref(n)))
    out = np.zeros(raw.size, dtype=[("job", "<u4"), ("prevSlot", "u1"), ("flags", "u1")])
    out["job"] = raw & 0xFFFFFFFF
    out["prevSlot"] = (raw >> 32) & 0xFF
    out["flags"] = (raw >> 40) & 0xFF
    return out.reshape(n.value, fpw)


def pack_chunks(blob, srcs, jobs, fpw, mids=None):
    """dcs_pack_chunks -> uint8 array [nChunks, packageBytes] (what a batch uploads for unpack round 0); mids: the sources' mid
    records (index_stream_mids), for the packages of the even deal (dcs_pack_chunks_mids)"""
    L = load_library()
    blob_a = np.frombuffer(bytes(blob), dtype=np.uint8)
    srcs = np.ascontiguousarray(srcs, dtype=SRC_DTYPE)
    jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
    n, pb = ctypes.c_uint32(0), ctypes.c_uint32(0)
    entry, with_mids = L.dcs_pack_chunks, ()
    if mids is not None:
        mids = np.ascontiguousarray(mids, dtype=np.uint32)
        assert mids.shape == (srcs.size, 16)
        entry, with_mids = L.dcs_pack_chunks_mids, (_ptr(mids),)

    def call(out, cap):
        return entry(_ptr(jobs), jobs.size, _ptr(srcs), *with_mids, _ptr(blob_a), blob_a.size, fpw, out, cap, ctypes.byref(n), ctypes.byref(pb))
    _check(call(None, 0))
    out = np.zeros((n.value, pb.value), dtype=np.uint8)
    _check(call(_ptr(out), out.size))
    return out


def even_deal_lane(n_bands, q):
    """dcs_even_deal_lane -> (first unit, units) of lane q of a frame of n_bands header bands, and the samples the deal saves"""
    first, count, gain = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    load_library().dcs_even_deal_lane(n_bands, q, ctypes.byref(first), ctypes.byref(count), ctypes.byref(gain))
    return first.value, count.value, gain.value


def prepass_short(n_bands):
    """dcs_prepass_short -> (steps of the 1994+ transform's pre-pass that have no partner in a row of n_bands header bands, the last
    tile word such a row can fill)"""
    last = ctypes.c_int(0)
    return load_library().dcs_prepass_short(n_bands, ctypes.byref(last)), last.value


def device_count():
    return load_library().dcs_device_count()


def host_threads():
    """dcs_host_threads: CPUs this process can really use (affinity mask, cgroup quota)"""
    return load_library().dcs_host_threads()


def partition_streams(frame_counts, n_parts):
    """dcs_partition_streams: cut points (n_parts + 1) of contiguous ranges balanced by total frame count"""
    fc = np.ascontiguousarray(frame_counts, dtype=np.uint32)
    cut = np.zeros(n_parts + 1, dtype=np.uint32)
    st = load_library().dcs_partition_streams(_ptr(fc), fc.size, n_parts, _ptr(cut))
    if st != 0:
        raise DcsError(st)
    return cut


def _stream_refs(streams):
    keep = [np.frombuffer(bytes(s[1]), dtype=np.uint8) for s in streams]
    refs = (StreamRef * len(streams))()
    for k, s in enumerate(streams):
        refs[k].data = keep[k].ctypes.data
        refs[k].len = keep[k].size
        refs[k].os = s[0]
        refs[k].volume = s[2]
        refs[k].level = s[3]
        refs[k].channelVolume = 0xFF
    return refs, keep


def decode_streams_sharded(device_ids, streams, extra_frames=0):
    """dcs_decode_streams_sharded: (os, bytes, volume, level) streams over several devices (one host thread and one
    context per device, range partition balanced by frames) -> (pcm [frames, 240], err, first frame of each stream,
    first stream of each device)"""
    L = load_library()
    streams = list(streams)
    refs, keep = _stream_refs(streams)
    total = int(sum(((int(k[0]) << 8) | int(k[1])) + extra_frames for k in keep))
    pcm = np.zeros((total, FRAME_SAMPLES), dtype=np.int16)
    err = np.zeros(total, dtype=np.uint32)
    first = np.zeros(len(streams) + 1, dtype=np.uint32)
    devs = np.ascontiguousarray(device_ids, dtype=np.int32)
    cut = np.zeros(devs.size + 1, dtype=np.uint32)
    st = L.dcs_decode_streams_sharded(_ptr(devs), devs.size, refs, len(streams), extra_frames, _ptr(pcm), total,
                                      _ptr(first), _ptr(err), _ptr(cut))
    if st != 0:
        msg = L.dcs_last_error(None)
        raise DcsError(st, msg.decode() if msg else "")
    return pcm, err, first, cut


# ---------------------------------------------------------------------------------------------- device side
class Context:
    """DcsCtx: one GPU.  Raises DcsError(DCS_ERR_NO_DEVICE) when there is no gfx950 device."""

    def __init__(self, device=0):
        self.L = load_library()
        h = ctypes.c_void_p()
        st = self.L.dcs_ctx_create(device, ctypes.byref(h))
        if st != 0:
            msg = self.L.dcs_last_error(None)
            raise DcsError(st, msg.decode() if msg else "")
        self.h = h
        self.device = int(device)
        self._batches = weakref.WeakSet()       # a DcsBatch must be destroyed before its DcsCtx (dcs_hip.h)

    def close(self):
        if self.h:
            for b in list(self._batches):
                b.close()
            self.L.dcs_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def link_rate(self):
        """GB/s, device memory -> pinned host memory, measured now (dcs_ctx_link_rate)"""
        v = ctypes.c_float(0)
        _check(self.L.dcs_ctx_link_rate(self.h, ctypes.byref(v)), self.h)
        return float(v.value)

    def set_concurrent_batches(self, enable=True):
        """batches created afterwards may run next to other decode launches on the GPU (dcs_ctx_set_concurrent_batches)"""
        _check(self.L.dcs_ctx_set_concurrent_batches(self.h, int(bool(enable))), self.h)

    def set_batch_tails(self, all_frames=True):
        """resident batches created afterwards store every frame's tail (True) or the last frame's of every chain (False, default)"""
        _check(self.L.dcs_ctx_set_batch_tails(self.h, int(bool(all_frames))), self.h)

    def set_cache_limits(self, device_bytes, pinned_bytes):
        _check(self.L.dcs_ctx_set_cache_limits(self.h, int(device_bytes), int(pinned_bytes)), self.h)

    def trim_cache(self):
        """release every cached buffer -> (device bytes, pinned bytes) released"""
        d, p = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(self.L.dcs_ctx_trim_cache(self.h, ctypes.byref(d), ctypes.byref(p)), self.h)
        return d.value, p.value

    def cache_bytes(self):
        """-> (device bytes cached, pinned bytes cached, device limit, pinned limit)"""
        v = [ctypes.c_uint64(0) for _ in range(4)]
        _check(self.L.dcs_ctx_cache_bytes(self.h, *[ctypes.byref(x) for x in v]), self.h)
        return tuple(x.value for x in v)

    def set_frames_per_wave(self, fpw):
        _check(self.L.dcs_ctx_set_frames_per_wave(self.h, fpw), self.h)

    def set_chunks_per_wave(self, chunks):
        """Chunks a wavefront of a decode launch takes, one after the other: 1, 2, or 0 for the library's rule (2 for batches
        of 8 frames per wavefront that make more than one and at most two generations of the chip).  Read at every launch."""
        _check(self.L.dcs_ctx_set_chunks_per_wave(self.h, chunks), self.h)

    def set_even_deal(self, mode):
        """The deal of 1994+ frames to their unpack lanes in batches created afterwards from descriptors with mid records:
        0 whole bands, 1 units of 8 samples wherever the batch allows it, -1 (default) units where some frame gains."""
        _check(self.L.dcs_ctx_set_even_deal(self.h, mode), self.h)

    def set_sole_source_kernel(self, mode):
        """The kernel of an even-deal batch none of whose jobs has a second source: -1 (default) the instantiation without the
        rounds of further sources, 0 never.  Read at every launch."""
        _check(self.L.dcs_ctx_set_sole_source_kernel(self.h, mode), self.h)

    def set_frames_per_chunk(self, frames):
        _check(self.L.dcs_ctx_set_frames_per_chunk(self.h, frames), self.h)

    def set_tail_handoff(self, enable):
        _check(self.L.dcs_ctx_set_tail_handoff(self.h, int(bool(enable))), self.h)

    def set_large_list_path(self, on_device, shared=True):
        """dcs_decode_streams on a large list: 0 = index pass on the host's pool; 1 = index walk, planner and packer on the device;
        2 (default) = the device path with the host pool walking the list's first parts next to the index kernel.
        on_device may also be the mode itself (0, 1, 2)."""
        mode = int(on_device) if on_device in (0, 1, 2) and not isinstance(on_device, bool) else (0 if not on_device else (2 if shared else 1))
        _check(self.L.dcs_ctx_set_large_list_path(self.h, mode), self.h)

    def decode_batch(self, blob, srcs, jobs, tails_in=None, want_tails=False):
        blob_a = np.frombuffer(bytes(blob), dtype=np.uint8)
        srcs = np.ascontiguousarray(srcs, dtype=SRC_DTYPE)
        jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
        n = jobs.size
        pcm = np.zeros((n, FRAME_SAMPLES), dtype=np.int16)
        err = np.zeros(n, dtype=np.uint32)
        tails = np.zeros((n, 16), dtype=np.int16) if want_tails else None
        tin = None if tails_in is None else np.ascontiguousarray(tails_in, dtype=np.int16)
        _check(self.L.dcs_decode_batch(self.h, _ptr(blob_a), blob_a.size, _ptr(srcs), srcs.size, _ptr(jobs), n,
                                       _ptr(tin), 0 if tin is None else tin.shape[0], _ptr(pcm), _ptr(err),
                                       _ptr(tails)), self.h)
        return (pcm, err, tails) if want_tails else (pcm, err)

    def call_floor(self, n_frames, iters=200):
        """dcs_ctx_call_floor -> (launch + wait, launch + copy of n_frames x 516 B + wait) in microseconds"""
        a, b = ctypes.c_float(), ctypes.c_float()
        _check(self.L.dcs_ctx_call_floor(self.h, n_frames, iters, ctypes.byref(a), ctypes.byref(b)), self.h)
        return a.value, b.value

    def decode_batch_live(self, blob, srcs, jobs, tails_in=None, blob_id=0):
        """dcs_decode_batch_live: the context's persistent small-batch decoder -> (pcm, err, tails), copies of what lies in the
        context's pinned memory until its next decode call"""
        blob_a = np.frombuffer(bytes(blob), dtype=np.uint8)
        srcs = np.ascontiguousarray(srcs, dtype=SRC_DTYPE)
        jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
        n = jobs.size
        tin = None if tails_in is None else np.ascontiguousarray(tails_in, dtype=np.int16)
        pcm, err, tails = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        _check(self.L.dcs_decode_batch_live(self.h, _ptr(blob_a), ctypes.c_size_t(blob_a.size), ctypes.c_uint64(blob_id), _ptr(srcs), srcs.size,
                                            _ptr(jobs), n, _ptr(tin), 0 if tin is None else tin.shape[0],
                                            ctypes.byref(pcm), ctypes.byref(err), ctypes.byref(tails)), self.h)
        def view(p, dtype, shape):
            nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
            return np.frombuffer(ctypes.string_at(p.value, nbytes), dtype=dtype).reshape(shape).copy()
        return view(pcm, np.int16, (n, FRAME_SAMPLES)), view(err, np.uint32, (n,)), view(tails, np.int16, (n, 16))

    def decode_streams(self, streams, extra_frames=0):
        """streams: iterable of (os, bytes, volume, level) -> (pcm [frames,240], err, first_job)"""
        b = build_stream_batch(streams, extra_frames)
        pcm, err = self.decode_batch(b["blob"], b["srcs"], b["jobs"])
        return pcm, err, b["first_job"]

    def batch(self, blob, srcs, jobs, tails_in=None, mids=None):
        """mids: the sources' mid records (build_stream_batch's "mids"; default: what `srcs` carries, if anything)"""
        return Batch(self, blob, srcs, jobs, tails_in, mids=mids)

    def encode_streams(self, pcm_list, fmt=None, **params):
        """dcs_encode_streams: PCM at 31 250 Hz (float32 in [-1, 1], or int16, which is divided by 32768) -> 1994+ streams,
        byte for byte the reference DCSEncoder's.  fmt: None = the reference's wildcard, or FMT_94_T0, FMT_94_T1_S0,
        FMT_94_T1_S3, FMT_94_T0_S3; params: CompressionParams fields by name.  Returns (list of bytes, ENCODE_INFO_DTYPE array)."""
        p = encode_params(fmt, **params)
        pcm, offs = _encode_input(pcm_list)
        n = len(offs) - 1
        out_offs = np.zeros(n + 1, np.uint64)
        info = np.zeros(n, ENCODE_INFO_DTYPE)
        cap = sum(encode_bound(offs[i + 1] - offs[i]) for i in range(n))
        out = np.zeros(max(cap, 1), np.uint8)
        _check(self.L.dcs_encode_streams(self.h, _ptr(pcm), _ptr(offs), n, ctypes.byref(p), _ptr(out), cap, _ptr(out_offs), _ptr(info)), self.h)
        return [out[out_offs[i]:out_offs[i + 1]].tobytes() for i in range(n)], info

    def encode_rd_streams(self, pcm_list, fmt=None, budget=None, **params):
        """dcs_encode_rd_streams: PCM at 31 250 Hz (as encode_streams) -> 1994+ streams from the rate-distortion search of
        DESIGN.md 10.11, each held to a budget.  fmt as encode_streams (None: every layout).  budget: None = the frame bits
        targetBitRate gives; an int = the most bytes any stream may have; a sequence = per stream.  Returns (list of bytes,
        ENCODE_INFO_DTYPE array, ENCODE_RD_INFO_DTYPE array)."""
        p = encode_params(fmt, **params)
        pcm, offs = _encode_input(pcm_list)
        n = len(offs) - 1
        bud = None
        if budget is not None:
            bud = np.ascontiguousarray(np.broadcast_to(np.asarray(budget, np.int64), (n,)).clip(0, 0xFFFFFFFF), dtype=np.uint32)
        out_offs = np.zeros(n + 1, np.uint64)
        info, info_rd = np.zeros(n, ENCODE_INFO_DTYPE), np.zeros(n, ENCODE_RD_INFO_DTYPE)
        cap = sum(encode_rd_bound(offs[i + 1] - offs[i]) for i in range(n))
        out = np.zeros(max(cap, 1), np.uint8)
        _check(self.L.dcs_encode_rd_streams(self.h, _ptr(pcm), _ptr(offs), n, ctypes.byref(p), _ptr(bud) if bud is not None and n else None,
                                            _ptr(out), cap, _ptr(out_offs), _ptr(info), _ptr(info_rd)), self.h)
        return [out[out_offs[i]:out_offs[i + 1]].tobytes() for i in range(n)], info, info_rd

    def encode93_rd_streams(self, pcm_list, os_=OS93B, budget=None, **params):
        """dcs_encode93_rd_streams: PCM at 31 250 Hz (as encode93_streams) -> OS93 Type-0 streams of os_ (OS93A or OS93B) from
        the rate-distortion search of DESIGN.md 10.12, each held to a budget.  budget: None = the frame bits targetBitRate
        gives; an int = the most bytes any stream may have; a sequence = per stream.  Returns (list of bytes,
        ENCODE_INFO_DTYPE array, ENCODE_RD_INFO_DTYPE array)."""
        if os_ not in _ENCODE93_VERSION:
            raise ValueError("encode93_rd_streams: os_ is OS93A or OS93B")
        p = encode_params(None, **dict(dict(formatVersion=_ENCODE93_VERSION[os_], streamFormatType=0, streamFormatSubType=0), **params))
        pcm, offs = _encode_input(pcm_list)
        n = len(offs) - 1
        bud = None
        if budget is not None:
            bud = np.ascontiguousarray(np.broadcast_to(np.asarray(budget, np.int64), (n,)).clip(0, 0xFFFFFFFF), dtype=np.uint32)
        out_offs = np.zeros(n + 1, np.uint64)
        info, info_rd = np.zeros(n, ENCODE_INFO_DTYPE), np.zeros(n, ENCODE_RD_INFO_DTYPE)
        cap = sum(encode93_rd_bound(offs[i + 1] - offs[i]) for i in range(n))
        out = np.zeros(max(cap, 1), np.uint8)
        _check(self.L.dcs_encode93_rd_streams(self.h, _ptr(pcm), _ptr(offs), n, ctypes.byref(p), _ptr(bud) if bud is not None and n else None,
                                              _ptr(out), cap, _ptr(out_offs), _ptr(info), _ptr(info_rd)), self.h)
        return [out[out_offs[i]:out_offs[i + 1]].tobytes() for i in range(n)], info, info_rd

    def _encode_rd_fit(self, entry, bound, p, pcm_list, total, cap):
        pcm, offs = _encode_input(pcm_list)
        n = len(offs) - 1
        caps = None
        if cap is not None:
            caps = np.ascontiguousarray(np.broadcast_to(np.asarray(cap, np.int64), (n,)).clip(0, 0xFFFFFFFF), dtype=np.uint32)
        out_offs = np.zeros(n + 1, np.uint64)
        info, info_rd = np.zeros(n, ENCODE_INFO_DTYPE), np.zeros(n, ENCODE_RD_INFO_DTYPE)
        fit = np.zeros(1, ENCODE_RD_FIT_INFO_DTYPE)
        room = sum(bound(offs[i + 1] - offs[i]) for i in range(n))
        out = np.zeros(max(room, 1), np.uint8)
        _check(entry(self.h, _ptr(pcm), _ptr(offs), n, ctypes.byref(p), int(total), _ptr(caps) if caps is not None and n else None,
                     _ptr(out), room, _ptr(out_offs), _ptr(info), _ptr(info_rd), _ptr(fit)), self.h)
        return [out[out_offs[i]:out_offs[i + 1]].tobytes() for i in range(n)], info, info_rd, fit[0]

    def encode_rd_fit(self, pcm_list, total, fmt=None, cap=None, **params):
        """dcs_encode_rd_fit: PCM as encode_rd_streams -> 1994+ streams that together take at most `total` bytes, the bytes
        dealt among them by the allocator of DESIGN.md 10.13.  cap: None, an int = the most bytes any stream may have, or a
        sequence = per stream.  Stream j is what encode_rd_streams writes for budget = its allotment, which is its length.
        Returns (list of bytes, ENCODE_INFO_DTYPE array, ENCODE_RD_INFO_DTYPE array, ENCODE_RD_FIT_INFO_DTYPE record)."""
        return self._encode_rd_fit(self.L.dcs_encode_rd_fit, encode_rd_bound, encode_params(fmt, **params), pcm_list, total, cap)

    def encode93_rd_fit(self, pcm_list, total, os_=OS93B, cap=None, **params):
        """dcs_encode93_rd_fit: encode_rd_fit for OS93 Type-0 streams of os_ (OS93A or OS93B), over encode93_rd_streams' search"""
        if os_ not in _ENCODE93_VERSION:
            raise ValueError("encode93_rd_fit: os_ is OS93A or OS93B")
        p = encode_params(None, **dict(dict(formatVersion=_ENCODE93_VERSION[os_], streamFormatType=0, streamFormatSubType=0), **params))
        return self._encode_rd_fit(self.L.dcs_encode93_rd_fit, encode93_rd_bound, p, pcm_list, total, cap)

    def encode_sweep(self, pcm_list, sets, jobs=None, measure=True, streams=True):
        """dcs_encode_sweep: jobs = (stream, set) pairs encoded in one call; sets = EncodeParams of one encoder (encode_params /
        encode93_params / transcode_params); jobs None = every pair, stream-major.  PCM as encode_streams.  measure: each
        job's stream is decoded on the device and compared with its source (SWEEP_RESULT_DTYPE's sums; sweep_sq_err).
        Returns (list of bytes per job, or None when streams is false; SWEEP_RESULT_DTYPE array)."""
        pcm, offs = _encode_input(pcm_list)
        n = len(offs) - 1
        arr = (EncodeParams * max(len(sets), 1))(*sets)
        if jobs is None:
            jl, n_jobs = None, n * len(sets)
        else:
            jl = np.zeros(max(len(jobs), 1), SWEEP_JOB_DTYPE)
            for k, (s, p) in enumerate(jobs):
                jl[k] = (s, p)
            n_jobs = len(jobs)
        res = np.zeros(max(n_jobs, 1), SWEEP_RESULT_DTYPE)
        out_offs = np.zeros(n_jobs + 1, np.uint64)
        flags = SWEEP_MEASURE if measure else 0
        args = (self.h, _ptr(pcm), _ptr(offs), n, arr, len(sets), _ptr(jl) if jl is not None else None, n_jobs, flags, _ptr(res))
        if not streams:
            _check(self.L.dcs_encode_sweep(*args, None, 0, _ptr(out_offs)), self.h)
            return None, res[:n_jobs]
        # sizes first would cost a second pass: the encoders' bound of every job's stream instead
        bound = encode_bound if len(sets) and sets[0].formatVersion == 0x9400 else encode93_bound
        each = [bound(int(offs[i + 1] - offs[i])) for i in range(n)]
        cap = sum(each) * len(sets) if jobs is None else sum(each[s] for s, _ in jobs if 0 <= s < n)
        out = np.zeros(max(cap, 1), np.uint8)
        _check(self.L.dcs_encode_sweep(*args, _ptr(out), cap, _ptr(out_offs)), self.h)
        return [out[out_offs[j]:out_offs[j + 1]].tobytes() for j in range(n_jobs)], res[:n_jobs]

    def encode_fit(self, pcm_list, sets, budget):
        """the best of `sets` (in order of preference) per stream within `budget` bytes: a measuring sweep without bytes,
        encode_fit_choose on its sizes and squared errors, then one job per stream for the bytes.  Returns (list of bytes,
        choice per stream, SWEEP_RESULT_DTYPE records of the chosen jobs, total bytes); raises DcsError status -5 (with
        `needed`) when no set fits as a whole."""
        n, k = len(pcm_list), len(sets)
        _, res = self.encode_sweep(pcm_list, sets, None, measure=True, streams=False)
        if not res["measured"].all():
            j = int(np.flatnonzero(res["measured"] == 0)[0])
            raise DcsError(-6, "stream %d, set %d: an OS93a stream with no band kept cannot be decoded, so not measured" % (j // k, j % k))
        n_bytes = res["enc"]["nBytes"].astype(np.uint64).reshape(n, k)
        sq_err = np.array(sweep_sq_err(res), dtype=np.uint64).reshape(n, k)
        choice, total = encode_fit_choose(n_bytes, sq_err, budget)
        out, _ = self.encode_sweep(pcm_list, sets, [(i, int(choice[i])) for i in range(n)], measure=False, streams=True)
        return out, choice, res.reshape(n, k)[np.arange(n), choice], total

    def encode93_streams(self, pcm_list, os_=OS93B, fmt=None, **params):
        """dcs_encode93_streams: PCM at 31 250 Hz (as encode_streams) -> OS93 streams, byte for byte the reference DCSEncoder's
        with formatVersion 0x9301 (os_=OS93A) or 0x9302 (OS93B).  fmt: None = the reference's wildcard, FMT_93_T0, FMT_93B_T1
        (OS93B only) or FMT_93A_T1 (OS93A only; the library refuses it, as the reference does).  Returns (list of bytes,
        ENCODE_INFO_DTYPE array)."""
        p = encode93_params(os_, fmt, **params)
        pcm, offs = _encode_input(pcm_list)
        n = len(offs) - 1
        out_offs = np.zeros(n + 1, np.uint64)
        info = np.zeros(n, ENCODE_INFO_DTYPE)
        cap = sum(encode93_bound(offs[i + 1] - offs[i]) for i in range(n))
        out = np.zeros(max(cap, 1), np.uint8)
        _check(self.L.dcs_encode93_streams(self.h, _ptr(pcm), _ptr(offs), n, ctypes.byref(p), _ptr(out), cap, _ptr(out_offs), _ptr(info)), self.h)
        return [out[out_offs[i]:out_offs[i + 1]].tobytes() for i in range(n)], info

    def encode93a_streams(self, pcm_list, fmt=None, **params):
        """dcs_encode93a_streams: PCM at 31 250 Hz (as encode_streams) -> OS93a streams (formatVersion 0x9301).  fmt:
        FMT_93A_T1 = the pair-table layout, which the reference cannot write (DESIGN.md 10.10 states the algorithm),
        FMT_93_T0 = the bytes encode93_streams gives, None = both and per stream the first strictly smallest, Type 0 first.
        Returns (list of bytes, ENCODE_INFO_DTYPE array, ENCODE93A_INFO_DTYPE array: the Type-1 candidate, zeros with FMT_93_T0)."""
        if fmt not in (None, FMT_93_T0, FMT_93A_T1):
            raise ValueError("no OS93a layout %r" % (fmt,))
        p = encode_params(None, **dict(dict(formatVersion=0x9301, streamFormatType=_ENCODE93_FMT[fmt], streamFormatSubType=-1), **params))
        pcm, offs = _encode_input(pcm_list)
        n = len(offs) - 1
        out_offs = np.zeros(n + 1, np.uint64)
        info, info_a = np.zeros(n, ENCODE_INFO_DTYPE), np.zeros(n, ENCODE93A_INFO_DTYPE)
        cap = sum(encode93a_bound(offs[i + 1] - offs[i]) for i in range(n))
        out = np.zeros(max(cap, 1), np.uint8)
        _check(self.L.dcs_encode93a_streams(self.h, _ptr(pcm), _ptr(offs), n, ctypes.byref(p), _ptr(out), cap, _ptr(out_offs), _ptr(info),
                                            _ptr(info_a)), self.h)
        return [out[out_offs[i]:out_offs[i + 1]].tobytes() for i in range(n)], info, info_a

    def encode93a_sweep(self, pcm_list, sets, jobs=None, measure=True, streams=True):
        """dcs_encode93a_sweep: encode_sweep for OS93a, whose sets (encode93a_params) may mix FMT_93_T0 and FMT_93A_T1; a
        Type-1 stream is searched once however many rates it is encoded at.  Returns (list of bytes per job, or None when
        streams is false; SWEEP_RESULT_DTYPE array; ENCODE93A_INFO_DTYPE array: the Type-1 candidate, zeros of a Type-0 job)."""
        pcm, offs = _encode_input(pcm_list)
        n = len(offs) - 1
        arr = (EncodeParams * max(len(sets), 1))(*sets)
        if jobs is None:
            jl, n_jobs = None, n * len(sets)
        else:
            jl = np.zeros(max(len(jobs), 1), SWEEP_JOB_DTYPE)
            for k, (s, p) in enumerate(jobs):
                jl[k] = (s, p)
            n_jobs = len(jobs)
        res = np.zeros(max(n_jobs, 1), SWEEP_RESULT_DTYPE)
        info_a = np.zeros(max(n_jobs, 1), ENCODE93A_INFO_DTYPE)
        out_offs = np.zeros(n_jobs + 1, np.uint64)
        flags = SWEEP_MEASURE if measure else 0
        args = (self.h, _ptr(pcm), _ptr(offs), n, arr, len(sets), _ptr(jl) if jl is not None else None, n_jobs, flags, _ptr(res),
                _ptr(info_a))
        if not streams:
            _check(self.L.dcs_encode93a_sweep(*args, None, 0, _ptr(out_offs)), self.h)
            return None, res[:n_jobs], info_a[:n_jobs]
        each = [encode93a_bound(int(offs[i + 1] - offs[i])) for i in range(n)]
        cap = sum(each) * len(sets) if jobs is None else sum(each[s] for s, _ in jobs if 0 <= s < n)
        out = np.zeros(max(cap, 1), np.uint8)
        _check(self.L.dcs_encode93a_sweep(*args, _ptr(out), cap, _ptr(out_offs)), self.h)
        return [out[out_offs[j]:out_offs[j + 1]].tobytes() for j in range(n_jobs)], res[:n_jobs], info_a[:n_jobs]

    def encode93a_fit(self, pcm_list, sets, budget):
        """encode_fit on encode93a_sweep: the best of `sets` (OS93a, either layout, in order of preference) per stream within
        `budget` bytes.  Returns (list of bytes, choice per stream, SWEEP_RESULT_DTYPE records of the chosen jobs, total
        bytes); raises DcsError status -5 (with `needed`) when no set fits as a whole."""
        n, k = len(pcm_list), len(sets)
        _, res, _ = self.encode93a_sweep(pcm_list, sets, None, measure=True, streams=False)
        if not res["measured"].all():
            j = int(np.flatnonzero(res["measured"] == 0)[0])
            raise DcsError(-6, "stream %d, set %d: an OS93a Type-0 stream with no band kept cannot be decoded, so not measured" % (j // k, j % k))
        n_bytes = res["enc"]["nBytes"].astype(np.uint64).reshape(n, k)
        sq_err = np.array(sweep_sq_err(res), dtype=np.uint64).reshape(n, k)
        choice, total = encode_fit_choose(n_bytes, sq_err, budget)
        out, _, _ = self.encode93a_sweep(pcm_list, sets, [(i, int(choice[i])) for i in range(n)], measure=False, streams=True)
        return out, choice, res.reshape(n, k)[np.arange(n), choice], total

    def level_streams(self, pcm_list, level):
        """dcs_level_streams: the level stage alone on PCM at 31 250 Hz (as encode_streams; a stream may be empty).  level: a
        Level for every stream, or a list with one per stream.  Returns (list of float32 arrays, LEVEL_INFO_DTYPE array)."""
        pcm, offs = _encode_input(pcm_list)
        n = len(offs) - 1
        lv, n_lv = _levels(level, n)
        out = np.zeros(max(int(offs[-1]), 1), np.float32)
        out_offs = np.zeros(n + 1, np.uint64)
        info = np.zeros(max(n, 1), LEVEL_INFO_DTYPE)
        _check(self.L.dcs_level_streams(self.h, _ptr(pcm), _ptr(offs), n, lv, n_lv, _ptr(out), out.size, _ptr(out_offs), _ptr(info)),
               self.h)
        return [out[out_offs[i]:out_offs[i + 1]].copy() for i in range(n)], info[:n]

    def resample_streams(self, pcm_list, rates, channels=1, filter=None, at_unity=False, level=None):
        """dcs_resample_streams: PCM at `rates` Hz (one rate, or one per stream; 4 000 .. 384 000) -> float32 at 31 250 Hz,
        what the reference's encoder feeds itself.  pcm_list: float32 arrays, or int16 arrays, which are divided by 32768;
        channels: 1 or 2 (interleaved, averaged), one value or one per stream; filter: None = the library's table, or
        (float32 coefficients, increment) in libsamplerate's layout; at_unity: run the converter at 31 250 Hz too.
        Returns a list of float32 arrays.  level: None, or a Level or a list of one per stream applied to the resampled
        signal (dcs_resample_streams_level); then the LEVEL_INFO_DTYPE array is returned as well, as the last element."""
        pcm, offs = _encode_input(pcm_list)
        n = len(offs) - 1
        r, ch = _per_stream(rates, n, np.uint32, "rates"), _per_stream(channels, n, np.int32, "channel counts")
        f, keep = _resample_filter(filter)
        flags = RESAMPLE_AT_UNITY if at_unity else 0
        fp = ctypes.byref(f) if f is not None else None
        out_offs = np.zeros(n + 1, np.uint64)
        out = np.zeros(max(sum(_resample_bound(int(offs[i + 1] - offs[i]), int(r[i]), int(ch[i]), at_unity) for i in range(n)), 1),
                       np.float32)
        args = (self.h, _ptr(pcm), _ptr(offs), n, _ptr(r), _ptr(ch), fp, flags, _ptr(out), out.size, _ptr(out_offs))
        if level is None:
            _check(self.L.dcs_resample_streams(*args), self.h)
            return [out[out_offs[i]:out_offs[i + 1]].copy() for i in range(n)]
        lv, n_lv = _levels(level, n)
        linfo = np.zeros(max(n, 1), LEVEL_INFO_DTYPE)
        _check(self.L.dcs_resample_streams_level(*args, lv, n_lv, _ptr(linfo)), self.h)
        del keep
        return [out[out_offs[i]:out_offs[i + 1]].copy() for i in range(n)], linfo[:n]

    def encode_streams_at(self, pcm_list, rates, version=0x9400, fmt=None, channels=1, filter=None, at_unity=False, level=None,
                          **params):
        """dcs_encode_streams_at: resample (as resample_streams), then encode on the device (version 0x9400: fmt as
        encode_streams; 0x9301 / 0x9302: fmt as encode93_streams), as the reference's EncodeFile does it for float input.
        Returns (list of bytes, ENCODE_INFO_DTYPE array); with level (as resample_streams) also the LEVEL_INFO_DTYPE array."""
        p = transcode_params(version, fmt, **params)
        pcm, offs = _encode_input(pcm_list)
        n = len(offs) - 1
        r, ch = _per_stream(rates, n, np.uint32, "rates"), _per_stream(channels, n, np.int32, "channel counts")
        f, keep = _resample_filter(filter)
        flags = RESAMPLE_AT_UNITY if at_unity else 0
        bound = encode_bound if version == 0x9400 else encode93_bound
        # no walk here: a bound on each stream's resampled length, and the encoder's bound of that (of the longest stream it
        # takes where the bound passes 65 535 frames: a longer stream is refused before its bytes are placed)
        cap = 0
        for i in range(n):
            m = _resample_bound(int(offs[i + 1] - offs[i]), int(r[i]), int(ch[i]), at_unity)
            cap += bound(m) or bound(65535 * 240)
        out = np.zeros(max(cap, 1), np.uint8)
        out_offs = np.zeros(n + 1, np.uint64)
        info = np.zeros(max(n, 1), ENCODE_INFO_DTYPE)
        args = (self.h, _ptr(pcm), _ptr(offs), n, _ptr(r), _ptr(ch), ctypes.byref(f) if f is not None else None, flags, ctypes.byref(p),
                _ptr(out), cap, _ptr(out_offs), _ptr(info))
        if level is None:
            _check(self.L.dcs_encode_streams_at(*args), self.h)
            return [out[out_offs[i]:out_offs[i + 1]].tobytes() for i in range(n)], info[:n]
        lv, n_lv = _levels(level, n)
        linfo = np.zeros(max(n, 1), LEVEL_INFO_DTYPE)
        _check(self.L.dcs_encode_streams_at_level(*args, lv, n_lv, _ptr(linfo)), self.h)
        del keep
        return [out[out_offs[i]:out_offs[i + 1]].tobytes() for i in range(n)], info[:n], linfo[:n]

    def wav_decode(self, files):
        """dcs_wav_decode: WAV files (bytes or paths) -> list of mono float32 arrays at each file's own rate, as libnyquist
        converts the samples and EncodeFile averages a stereo pair"""
        blob, offs = _files_blob(files)
        n = len(offs) - 1
        out_offs = np.zeros(n + 1, np.uint64)
        total = 0
        for i in range(n):
            w = wav_parse(blob[int(offs[i]):int(offs[i + 1])].tobytes())
            total += (w["nValues"] + 1) // 2 if w["channels"] == 2 else w["nValues"]
        out = np.zeros(max(total, 1), np.float32)
        _check(self.L.dcs_wav_decode(self.h, _ptr(blob), _ptr(offs), n, _ptr(out), out.size, _ptr(out_offs)), self.h)
        return [out[out_offs[i]:out_offs[i + 1]].copy() for i in range(n)]

    def flac_decode(self, files):
        """dcs_flac_decode: FLAC files (bytes or paths) -> list of mono float32 arrays at each file's own rate, as libnyquist's
        FlacDecoder converts libFLAC's samples and EncodeFile averages a stereo pair"""
        blob, offs = _files_blob(files)
        n = len(offs) - 1
        out_offs = np.zeros(n + 1, np.uint64)
        total = sum(flac_parse(blob[int(offs[i]):int(offs[i + 1])].tobytes())["totalSamples"] for i in range(n))
        out = np.zeros(max(total, 1), np.float32)
        _check(self.L.dcs_flac_decode(self.h, _ptr(blob), _ptr(offs), n, _ptr(out), out.size, _ptr(out_offs)), self.h)
        return [out[out_offs[i]:out_offs[i + 1]].copy() for i in range(n)]

    def _flac_written(self, call, n, cap):
        """the writer's capacity protocol: one call with the bound's capacity -> (list of bytes, FLAC_WRITE_INFO_DTYPE array)"""
        out = np.zeros(max(cap, 1), np.uint8)
        out_offs = np.zeros(n + 1, np.uint64)
        info = np.zeros(max(n, 1), FLAC_WRITE_INFO_DTYPE)
        _check(call(_ptr(out), cap, _ptr(out_offs), _ptr(info)), self.h)
        return [out[int(out_offs[i]):int(out_offs[i + 1])].tobytes() for i in range(n)], info[:n]

    def flac_write_streams(self, pcm_list, rate=31250, md5=True):
        """dcs_flac_write_streams: int16 PCM streams (whole frames of 240 samples) -> (list of FLAC streams as bytes,
        FLAC_WRITE_INFO_DTYPE array); mono, 16 bits, block size 4096, the MD5 of the samples in STREAMINFO if md5"""
        arrs = [np.ascontiguousarray(p, np.int16).ravel() for p in pcm_list]
        n = len(arrs)
        offs = np.zeros(n + 1, np.uint64)
        offs[1:] = np.cumsum([a.size for a in arrs], dtype=np.uint64)
        pcm = np.concatenate(arrs) if n else np.zeros(1, np.int16)
        cap = sum(flac_write_bound(a.size) for a in arrs)
        flags = FLAC_MD5 if md5 else 0
        return self._flac_written(lambda *o: self.L.dcs_flac_write_streams(self.h, _ptr(pcm), _ptr(offs), n, rate, flags, *o), n, cap)

    def flac_write_samples(self, pcm_list, rate, md5=True):
        """dcs_flac_write_samples: flac_write_streams for int16 PCM streams of any length from 1 sample on -> (list of FLAC
        streams as bytes, FLAC_WRITE_INFO_DTYPE array); streams of whole frames get flac_write_streams' bytes"""
        arrs = [np.ascontiguousarray(p, np.int16).ravel() for p in pcm_list]
        n = len(arrs)
        offs = np.zeros(n + 1, np.uint64)
        offs[1:] = np.cumsum([a.size for a in arrs], dtype=np.uint64)
        pcm = np.concatenate(arrs) if n else np.zeros(1, np.int16)
        cap = sum(flac_write_bound(a.size) for a in arrs)
        flags = FLAC_MD5 if md5 else 0
        return self._flac_written(lambda *o: self.L.dcs_flac_write_samples(self.h, _ptr(pcm), _ptr(offs), n, int(rate), flags, *o), n, cap)

    def _decode_refs_flac_at(self, refs, n, frames, rate, extra_frames, filter, flags):
        total = int(sum(frames)) + n * extra_frames
        err = np.zeros(max(total, 1), np.uint32)
        first = np.zeros(n + 1, np.uint32)
        first[1:] = np.cumsum([f + extra_frames for f in frames])
        f, keep = _resample_filter(filter)
        fp = ctypes.byref(f) if f is not None else None
        cap = sum(flac_write_bound(_resample_out_bound(int(fr + extra_frames) * FRAME_SAMPLES, int(rate), bool(flags & FLAC_AT_UNITY)))
                  for fr in frames)
        rate_info = np.zeros(max(n, 1), RATE_INFO_DTYPE)
        out, info = self._flac_written(lambda o, c, oo, i: self.L.dcs_decode_streams_flac_at(
            self.h, refs, n, extra_frames, int(rate), fp, flags, o, c, oo, i, _ptr(rate_info), _ptr(err)), n, cap)
        del keep
        return out, info, rate_info[:n], err[:total], first

    def decode_streams_flac_at(self, streams, rate, extra_frames=0, md5=True, filter=None, at_unity=False, sequence=False):
        """dcs_decode_streams_flac_at: decode_streams_at whose converted samples stay on the device and leave it as FLAC at
        `rate` Hz -> (list of FLAC streams as bytes, FLAC_WRITE_INFO_DTYPE array, RATE_INFO_DTYPE array, err, first_job);
        the bytes are flac_write_samples' of decode_streams_at's samples, everything else is decode_streams_at's"""
        streams = list(streams)
        refs, keep = _stream_refs(streams)
        frames = [(int(k[0]) << 8) | int(k[1]) for k in keep]
        flags = (FLAC_MD5 if md5 else 0) | (FLAC_AT_UNITY if at_unity else 0) | (FLAC_SEQUENCE if sequence else 0)
        return self._decode_refs_flac_at(refs, len(streams), frames, rate, extra_frames, filter, flags)

    def extract_streams_flac_at(self, romset, rate, volume=255, extra_frames=2, md5=True, filter=None, at_unity=False):
        """extract_streams whose PCM leaves the device as FLAC at `rate` Hz: -> (plan items, list of FLAC streams as bytes,
        FLAC_WRITE_INFO_DTYPE array, RATE_INFO_DTYPE array, first frame of each stream)"""
        items = romset.extract_plan()
        refs = romset.stream_refs(items, volume)
        frames = []
        for k in range(len(items)):
            one = ctypes.c_uint64()
            st = self.L.dcs_count_stream_frames(ctypes.byref(refs[k]), 1, 0, ctypes.byref(one))
            if st != 0:
                raise DcsError(st)
            frames.append(one.value)
        flags = FLAC_SEQUENCE | (FLAC_MD5 if md5 else 0) | (FLAC_AT_UNITY if at_unity else 0)
        out, info, rate_info, _, first = self._decode_refs_flac_at(refs, len(items), frames, rate, extra_frames, filter, flags)
        return items, out, info, rate_info, first

    def _decode_refs_flac(self, refs, n, frames, extra_frames, flags):
        total = int(sum(frames)) + n * extra_frames
        err = np.zeros(max(total, 1), np.uint32)
        first = np.zeros(n + 1, np.uint32)
        first[1:] = np.cumsum([f + extra_frames for f in frames])
        cap = sum(flac_write_bound((f + extra_frames) * FRAME_SAMPLES) for f in frames)
        out, info = self._flac_written(lambda *o: self.L.dcs_decode_streams_flac(self.h, refs, n, extra_frames, flags, *o, _ptr(err)), n, cap)
        return out, info, err[:total], first

    def decode_streams_flac(self, streams, extra_frames=0, md5=True):
        """dcs_decode_streams_flac: (os, bytes, volume, level) streams decoded as decode_streams decodes them, the PCM kept on
        the device and written as FLAC at 31 250 Hz there -> (list of FLAC streams as bytes, FLAC_WRITE_INFO_DTYPE array, err,
        first_job)"""
        streams = list(streams)
        refs, keep = _stream_refs(streams)
        frames = [(int(k[0]) << 8) | int(k[1]) for k in keep]
        return self._decode_refs_flac(refs, len(streams), frames, extra_frames, FLAC_MD5 if md5 else 0)

    def extract_streams_flac(self, romset, volume=255, extra_frames=2, md5=True):
        """extract_streams whose PCM leaves the device as FLAC: -> (plan items, list of FLAC streams as bytes,
        FLAC_WRITE_INFO_DTYPE array, first frame of each stream)"""
        items = romset.extract_plan()
        refs = romset.stream_refs(items, volume)
        frames = []
        for k in range(len(items)):
            one = ctypes.c_uint64()
            st = self.L.dcs_count_stream_frames(ctypes.byref(refs[k]), 1, 0, ctypes.byref(one))
            if st != 0:
                raise DcsError(st)
            frames.append(one.value)
        out, info, _, first = self._decode_refs_flac(refs, len(items), frames, extra_frames, FLAC_SEQUENCE | (FLAC_MD5 if md5 else 0))
        return items, out, info, first

    def resample_out_streams(self, pcm_list, rate, filter=None, at_unity=False):
        """dcs_resample_out_streams: int16 PCM streams at 31 250 Hz (any length >= 1) -> (list of int16 arrays at `rate` Hz,
        RATE_INFO_DTYPE array): libsamplerate's sinc converter at rate / 31250.0 between its own int16 conversions.  rate:
        4 000 .. 65 535, one per call; filter: None = the library's table, or (float32 coefficients, increment); 31 250
        returns the samples untouched unless at_unity."""
        arrs = [np.ascontiguousarray(p, np.int16).ravel() for p in pcm_list]
        n = len(arrs)
        offs = np.zeros(n + 1, np.uint64)
        offs[1:] = np.cumsum([a.size for a in arrs], dtype=np.uint64)
        pcm = np.concatenate(arrs) if n else np.zeros(1, np.int16)
        f, keep = _resample_filter(filter)
        fp = ctypes.byref(f) if f is not None else None
        flags = RESAMPLE_AT_UNITY if at_unity else 0
        cap = sum(_resample_out_bound(a.size, int(rate), at_unity) for a in arrs)
        out = np.zeros(max(cap, 1), np.int16)
        out_offs = np.zeros(n + 1, np.uint64)
        info = np.zeros(max(n, 1), RATE_INFO_DTYPE)
        _check(self.L.dcs_resample_out_streams(self.h, _ptr(pcm), _ptr(offs), n, int(rate), fp, flags, _ptr(out), cap, _ptr(out_offs),
                                               _ptr(info)), self.h)
        del keep
        return [out[int(out_offs[i]):int(out_offs[i + 1])].copy() for i in range(n)], info[:n]

    def _decode_refs_at(self, refs, n, frames, rate, extra_frames, filter, flags):
        total = int(sum(frames)) + n * extra_frames
        err = np.zeros(max(total, 1), np.uint32)
        first = np.zeros(n + 1, np.uint32)
        first[1:] = np.cumsum([f + extra_frames for f in frames])
        f, keep = _resample_filter(filter)
        fp = ctypes.byref(f) if f is not None else None
        cap = sum(_resample_out_bound(int(fr + extra_frames) * FRAME_SAMPLES, int(rate), bool(flags & RESAMPLE_AT_UNITY)) for fr in frames)
        out = np.zeros(max(cap, 1), np.int16)
        out_offs = np.zeros(n + 1, np.uint64)
        info = np.zeros(max(n, 1), RATE_INFO_DTYPE)
        _check(self.L.dcs_decode_streams_at(self.h, refs, n, extra_frames, int(rate), fp, flags, _ptr(out), cap, _ptr(out_offs),
                                            _ptr(info), _ptr(err)), self.h)
        del keep
        return [out[int(out_offs[i]):int(out_offs[i + 1])].copy() for i in range(n)], info[:n], err[:total], first

    def decode_streams_at(self, streams, rate, extra_frames=0, filter=None, at_unity=False, sequence=False):
        """dcs_decode_streams_at: (os, bytes, volume, level) streams decoded as decode_streams decodes them (sequence: as
        decode_stream_sequence does, one decoder object for the list), the PCM converted to `rate` Hz where it lies on the
        device (as resample_out_streams converts it) -> (list of int16 arrays, RATE_INFO_DTYPE array, err, first_job); err
        and first_job count decoded frames, as decode_streams gives them"""
        streams = list(streams)
        refs, keep = _stream_refs(streams)
        frames = [(int(k[0]) << 8) | int(k[1]) for k in keep]
        flags = (RESAMPLE_AT_UNITY if at_unity else 0) | (OUT_SEQUENCE if sequence else 0)
        return self._decode_refs_at(refs, len(streams), frames, rate, extra_frames, filter, flags)

    def extract_streams_at(self, romset, rate, volume=255, extra_frames=2, filter=None, at_unity=False):
        """extract_streams whose PCM leaves the device at `rate` Hz: -> (plan items, list of int16 arrays, RATE_INFO_DTYPE
        array, first frame of each stream)"""
        items = romset.extract_plan()
        refs = romset.stream_refs(items, volume)
        frames = []
        for k in range(len(items)):
            one = ctypes.c_uint64()
            st = self.L.dcs_count_stream_frames(ctypes.byref(refs[k]), 1, 0, ctypes.byref(one))
            if st != 0:
                raise DcsError(st)
            frames.append(one.value)
        out, info, _, first = self._decode_refs_at(refs, len(items), frames, rate, extra_frames, filter,
                                                   OUT_SEQUENCE | (RESAMPLE_AT_UNITY if at_unity else 0))
        return items, out, info, first

    def encode_files(self, files, version=0x9400, fmt=None, filter=None, at_unity=False, level=None, **params):
        """dcs_encode_files: DCSEncoder::EncodeFile on each file (bytes or paths): a DCSa container is copied or re-encoded as
        transcode_dcsa does it, a WAV or native FLAC file is read as libnyquist reads it, resampled and encoded (version, fmt, params as
        encode_streams_at).  Returns (list of stream bytes, ENCODE_FILE_INFO_DTYPE array); with level (a Level, or a list of
        one per file; WAV and FLAC files only) also the LEVEL_INFO_DTYPE array."""
        p = transcode_params(version, fmt, **params)
        blob, offs = _files_blob(files)
        n = len(offs) - 1
        f, keep = _resample_filter(filter)
        fp = ctypes.byref(f) if f is not None else None
        flags = RESAMPLE_AT_UNITY if at_unity else 0
        bound = np.zeros(max(n, 1), np.uint64)
        # (a file the plan refuses: the call below refuses it too, and names the reason in dcs_last_error)
        st = self.L.dcs_encode_files_plan(_ptr(blob), _ptr(offs), n, ctypes.byref(p), fp, flags, None, _ptr(bound), None)
        cap = int(bound[:n].sum()) if st == 0 else 0
        out = np.zeros(max(cap, 1), np.uint8)
        out_offs = np.zeros(n + 1, np.uint64)
        info = np.zeros(max(n, 1), ENCODE_FILE_INFO_DTYPE)
        args = (self.h, _ptr(blob), _ptr(offs), n, ctypes.byref(p), fp, flags, _ptr(out), cap, _ptr(out_offs), _ptr(info))
        if level is None:
            _check(self.L.dcs_encode_files(*args), self.h)
            return [out[out_offs[i]:out_offs[i + 1]].tobytes() for i in range(n)], info[:n]
        lv, n_lv = _levels(level, n)
        linfo = np.zeros(max(n, 1), LEVEL_INFO_DTYPE)
        _check(self.L.dcs_encode_files_level(*args, lv, n_lv, _ptr(linfo)), self.h)
        del keep
        return [out[out_offs[i]:out_offs[i + 1]].tobytes() for i in range(n)], info[:n], linfo[:n]

    def transcode_streams(self, streams, os_list, version=0x9400, fmt=None, reencode_all=False, volume=0x67, level=0xFF,
                          channel_volume=0xFF, **params):
        """dcs_transcode_streams: DCS streams (bytes; os_list[i] = the OS stream i plays under) into the family of `version`
        (0x9400, 0x9301 or 0x9302), as the reference's EncodeDCSFile does it: a stream that fits is copied, any other one is
        decoded (volume / level / channel_volume: the reference's 0x67 / 0xFF / 0xFF) and encoded again on the device.
        fmt and params: the target layout and CompressionParams (transcode_params).  Returns (list of bytes,
        TRANSCODE_INFO_DTYPE array)."""
        p = transcode_params(version, fmt, **params)
        flags = TRANSCODE_REENCODE_ALL if reencode_all else 0
        refs, keep = _transcode_refs(streams, os_list, volume, level, channel_volume)
        n = len(keep) if streams else 0
        bound = np.zeros(max(n, 1), np.uint64)
        # (a source the plan refuses: the call below refuses it too, and names the reason in dcs_last_error)
        st = self.L.dcs_transcode_plan(refs, n, ctypes.byref(p), flags, None, _ptr(bound))
        cap = int(bound[:n].sum()) if st == 0 else 0
        out = np.zeros(max(cap, 1), np.uint8)
        out_offs = np.zeros(n + 1, np.uint64)
        info = np.zeros(max(n, 1), TRANSCODE_INFO_DTYPE)
        _check(self.L.dcs_transcode_streams(self.h, refs, n, ctypes.byref(p), flags, _ptr(out), cap, _ptr(out_offs), _ptr(info)), self.h)
        return [out[out_offs[i]:out_offs[i + 1]].tobytes() for i in range(n)], info[:n]

    # ---- budgets from any source.  budget: None = the frame bits targetBitRate gives, an int or a sequence =
    # the most bytes per job; total: not None selects the shared form, all jobs together at most `total` bytes, with cap None,
    # an int or a sequence.  The shared form returns the ENCODE_RD_FIT_INFO_DTYPE record as well, as the last element.

    def encode_streams_at_budget(self, pcm_list, rates, version=0x9400, fmt=None, budget=None, total=None, cap=None, channels=1,
                                 filter=None, at_unity=False, level=None, **params):
        """dcs_encode_streams_at_budget: encode_streams_at with the searched encoder (encode_rd_streams / encode93_rd_streams,
        or encode_rd_fit / encode93_rd_fit with total) behind the level stage.  Returns (list of bytes, ENCODE_INFO_DTYPE
        array, ENCODE_RD_INFO_DTYPE array[, LEVEL_INFO_DTYPE array with level][, the fit record with total])."""
        p = transcode_params(version, fmt, **params)
        pcm, offs = _encode_input(pcm_list)
        n = len(offs) - 1
        r, ch = _per_stream(rates, n, np.uint32, "rates"), _per_stream(channels, n, np.int32, "channel counts")
        f, keep = _resample_filter(filter)
        flags = RESAMPLE_AT_UNITY if at_unity else 0
        bound = encode_rd_bound if version == 0x9400 else encode93_rd_bound
        room = 0
        for i in range(n):
            m = _resample_bound(int(offs[i + 1] - offs[i]), int(r[i]), int(ch[i]), at_unity)
            room += bound(m) or bound(65535 * 240)
        b, fit, alive = _budget(n, budget, total, cap)
        out = np.zeros(max(room, 1), np.uint8)
        out_offs = np.zeros(n + 1, np.uint64)
        info, info_rd = np.zeros(max(n, 1), ENCODE_INFO_DTYPE), np.zeros(max(n, 1), ENCODE_RD_INFO_DTYPE)
        lv, n_lv = _levels(level, n) if level is not None else (None, 0)
        linfo = np.zeros(max(n, 1), LEVEL_INFO_DTYPE)
        _check(self.L.dcs_encode_streams_at_budget(self.h, _ptr(pcm), _ptr(offs), n, _ptr(r), _ptr(ch), ctypes.byref(f) if f is not None else None,
                                                   flags, ctypes.byref(p), ctypes.byref(b), _ptr(out), room, _ptr(out_offs), _ptr(info),
                                                   _ptr(info_rd), lv, n_lv, _ptr(linfo) if level is not None else None), self.h)
        del keep, alive
        res = ([out[out_offs[i]:out_offs[i + 1]].tobytes() for i in range(n)], info[:n], info_rd[:n])
        return res + ((linfo[:n],) if level is not None else ()) + ((fit[0],) if total is not None else ())

    def transcode_streams_budget(self, streams, os_list, version=0x9400, fmt=None, reencode_all=False, budget=None, total=None,
                                 cap=None, volume=0x67, level=0xFF, channel_volume=0xFF, **params):
        """dcs_transcode_streams_budget: transcode_streams with the searched encoder behind the decode; a source that fits the
        target's family is still copied where it keeps to its own budget (or cap).  Returns (list of bytes,
        TRANSCODE_INFO_DTYPE array, ENCODE_RD_INFO_DTYPE array[, the fit record with total])."""
        p = transcode_params(version, fmt, **params)
        flags = TRANSCODE_REENCODE_ALL if reencode_all else 0
        refs, keep = _transcode_refs(streams, os_list, volume, level, channel_volume)
        n = len(keep) if streams else 0
        b, fit, alive = _budget(n, budget, total, cap)
        bound = np.zeros(max(n, 1), np.uint64)
        # (a source the plan refuses: the call below refuses it too, and names the reason in dcs_last_error)
        st = self.L.dcs_transcode_plan_budget(refs, n, ctypes.byref(p), flags, ctypes.byref(b), None, _ptr(bound))
        room = int(bound[:n].sum()) if st == 0 else 0
        out = np.zeros(max(room, 1), np.uint8)
        out_offs = np.zeros(n + 1, np.uint64)
        info, info_rd = np.zeros(max(n, 1), TRANSCODE_INFO_DTYPE), np.zeros(max(n, 1), ENCODE_RD_INFO_DTYPE)
        _check(self.L.dcs_transcode_streams_budget(self.h, refs, n, ctypes.byref(p), flags, ctypes.byref(b), _ptr(out), room, _ptr(out_offs),
                                                   _ptr(info), _ptr(info_rd)), self.h)
        del alive
        res = ([out[out_offs[i]:out_offs[i + 1]].tobytes() for i in range(n)], info[:n], info_rd[:n])
        return res + ((fit[0],) if total is not None else ())

    def encode_files_budget(self, files, version=0x9400, fmt=None, reencode_all=False, budget=None, total=None, cap=None,
                            filter=None, at_unity=False, level=None, **params):
        """dcs_encode_files_budget: encode_files with the searched encoder: WAV and FLAC files as encode_streams_at_budget,
        DCSa containers as transcode_streams_budget (reencode_all: every container is searched), the whole list in one
        search.  Returns (list of stream bytes, ENCODE_FILE_INFO_DTYPE array, ENCODE_RD_INFO_DTYPE array[, LEVEL_INFO_DTYPE
        array with level][, the fit record with total])."""
        p = transcode_params(version, fmt, **params)
        blob, offs = _files_blob(files)
        n = len(offs) - 1
        f, keep = _resample_filter(filter)
        fp = ctypes.byref(f) if f is not None else None
        rs_flags = RESAMPLE_AT_UNITY if at_unity else 0
        flags = rs_flags | (FILES_REENCODE_ALL if reencode_all else 0)
        b, fit, alive = _budget(n, budget, total, cap)
        bound = np.zeros(max(n, 1), np.uint64)
        # (a file the plan refuses: the call below refuses it too, and names the reason in dcs_last_error)
        st = self.L.dcs_encode_files_plan_budget(_ptr(blob), _ptr(offs), n, ctypes.byref(p), fp, flags, ctypes.byref(b), None, _ptr(bound))
        room = int(bound[:n].sum()) if st == 0 else 0
        out = np.zeros(max(room, 1), np.uint8)
        out_offs = np.zeros(n + 1, np.uint64)
        info, info_rd = np.zeros(max(n, 1), ENCODE_FILE_INFO_DTYPE), np.zeros(max(n, 1), ENCODE_RD_INFO_DTYPE)
        lv, n_lv = _levels(level, n) if level is not None else (None, 0)
        linfo = np.zeros(max(n, 1), LEVEL_INFO_DTYPE)
        _check(self.L.dcs_encode_files_budget(self.h, _ptr(blob), _ptr(offs), n, ctypes.byref(p), fp,
                                              flags, ctypes.byref(b), _ptr(out), room,
                                              _ptr(out_offs), _ptr(info), _ptr(info_rd), lv, n_lv,
                                              _ptr(linfo) if level is not None else None), self.h)
        del keep, alive
        res = ([out[out_offs[i]:out_offs[i + 1]].tobytes() for i in range(n)], info[:n], info_rd[:n])
        return res + ((linfo[:n],) if level is not None else ()) + ((fit[0],) if total is not None else ())

    def transcode_dcsa(self, containers, version=0x9400, fmt=None, reencode_all=False, **kw):
        """transcode_streams on "DCSa" containers (what EncodeDCSFile reads; the source OS from the container, 0x9400 as
        OS94) -> (list of containers in the target's version, TRANSCODE_INFO_DTYPE array)"""
        parsed = [dcsa_parse(c) for c in containers]
        out, info = self.transcode_streams([s for _, s in parsed], [o for o, _ in parsed], version, fmt, reencode_all, **kw)
        return [dcsa_header(TRANSCODE_OS[version], len(s)) + s for s in out], info

    def extract_streams(self, romset, volume=255, extra_frames=2):
        """the whole `--extract-streams` pipeline: ROM set -> plan -> one launch -> PCM per stream.
        -> (plan items, pcm [frames, 240], first frame of each stream)"""
        items = romset.extract_plan()
        refs = romset.stream_refs(items, volume)
        total = ctypes.c_uint64()
        st = self.L.dcs_count_stream_frames(refs, len(items), extra_frames, ctypes.byref(total))
        if st != 0:
            raise DcsError(st)
        pcm = np.zeros((total.value, FRAME_SAMPLES), dtype=np.int16)
        first = np.zeros(len(items) + 1, dtype=np.uint32)
        _check(self.L.dcs_decode_stream_sequence(self.h, refs, len(items), extra_frames, _ptr(pcm), total.value,
                                                 _ptr(first), None), self.h)
        return items, pcm, first

    def decode_stream_sequence(self, os_, volume, streams, levels, extra_frames=2):
        """dcs_decode_stream_sequence: the --extract-streams loop on one decoder object.
        streams: list of bytes; -> (pcm [frames, 240], err, first frame of each stream)"""
        keep = [np.frombuffer(bytes(s), dtype=np.uint8) for s in streams]
        refs = (StreamRef * len(streams))()
        total = 0
        for k, s in enumerate(keep):
            refs[k].data = s.ctypes.data
            refs[k].len = s.size
            refs[k].os = os_
            refs[k].volume = volume
            refs[k].level = levels[k]
            refs[k].channelVolume = 0xFF
            total += ((int(s[0]) << 8) | int(s[1])) + extra_frames
        pcm = np.zeros((total, FRAME_SAMPLES), dtype=np.int16)
        err = np.zeros(total, dtype=np.uint32)
        first = np.zeros(len(streams) + 1, dtype=np.uint32)
        _check(self.L.dcs_decode_stream_sequence(self.h, refs, len(streams), extra_frames, _ptr(pcm), total,
                                                 _ptr(first), _ptr(err)), self.h)
        return pcm, err, first

    def extract_tracks(self, romset, plan):
        """dcs_extract_tracks: the --extract-tracks loop on one decoder, every tick planned ahead on the host sequencer,
        one launch.  plan: [(track, frames)] (RomSet.extract_tracks_plan); -> (pcm [frames, 240], first frame of each track)"""
        items = np.array(plan, dtype=np.uint32).reshape(-1, 2)
        total = int(items[:, 1].sum()) if len(plan) else 0
        pcm = np.zeros((max(total, 1), FRAME_SAMPLES), dtype=np.int16)
        first = np.zeros(len(plan) + 1, dtype=np.uint32)
        _check(self.L.dcs_extract_tracks(self.h, romset.h, _ptr(items), len(plan), _ptr(pcm), total, _ptr(first), None), self.h)
        return pcm[:total], first

    def clock_mhz(self):
        """dcs_ctx_clock_mhz: the shader clock under an integer load on every SIMD (probe kernel)"""
        mhz = ctypes.c_float()
        _check(self.L.dcs_ctx_clock_mhz(self.h, ctypes.byref(mhz)), self.h)
        return mhz.value

    def set_test_hooks(self, chunk_order_seed=0, no_xcd_ranges=False):
        """test hooks: host-planned batches get their chunks in a seeded random order; no batch is launched in XCD ranges"""
        _check(self.L.dcs_ctx_set_test_hooks(self.h, int(chunk_order_seed), int(bool(no_xcd_ranges))), self.h)

    def device_path(self, streams, extra_frames=0):
        return DevicePath(self, streams, extra_frames)

    def pipeline(self, depth=3, index_on_device=False, pack_on_device=False, plan_on_device=False, flac=False, md5=True):
        return Pipeline(self, depth, index_on_device, pack_on_device, plan_on_device, flac, md5)

    def pack_chunks_device(self, blob, srcs, jobs, fpw):
        """dcs_pack_chunks_device -> uint8 array [nChunks, packageBytes], assembled by the device packer"""
        blob_a = np.frombuffer(bytes(blob), dtype=np.uint8)
        srcs = np.ascontiguousarray(srcs, dtype=SRC_DTYPE)
        jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
        n, pb = ctypes.c_uint32(0), ctypes.c_uint32(0)
        _check(self.L.dcs_pack_chunks_device(self.h, _ptr(jobs), jobs.size, _ptr(srcs), srcs.size, _ptr(blob_a), blob_a.size, fpw,
                                             None, 0, ctypes.byref(n), ctypes.byref(pb)), self.h)
        out = np.zeros((n.value, pb.value), dtype=np.uint8)
        _check(self.L.dcs_pack_chunks_device(self.h, _ptr(jobs), jobs.size, _ptr(srcs), srcs.size, _ptr(blob_a), blob_a.size, fpw,
                                             _ptr(out), out.size, ctypes.byref(n), ctypes.byref(pb)), self.h)
        return out

    def index_streams_gpu(self, streams):
        """dcs_index_streams_gpu: the index pass on the GPU, one wavefront per stream.  Same result as
        index_streams / index_stream."""
        streams = list(streams)
        if not streams:
            return []
        blob, locs = pack_streams(streams)
        counts = _frame_counts(streams)
        cap = int(counts.sum())
        out = np.zeros(max(cap, 1), dtype=INDEX_DTYPE)
        infos = np.zeros(len(streams), dtype=INFO_DTYPE)
        b = np.frombuffer(blob, dtype=np.uint8)
        _check(self.L.dcs_index_streams_gpu(self.h, _ptr(b), b.size, _ptr(locs), len(streams), _ptr(out), cap,
                                            _ptr(infos)), self.h)
        return _split_records(out, infos, locs["firstRecord"])

    def index_gpu_time(self, iters=10):
        ms = ctypes.c_float()
        _check(self.L.dcs_index_streams_gpu_time(self.h, iters, ctypes.byref(ms)), self.h)
        return ms.value


class Batch:
    """DcsBatch: a job list resident in HBM"""

    def __init__(self, ctx, blob, srcs, jobs, tails_in=None, mids=None):
        self.ctx = ctx
        self.L = ctx.L
        blob_a = np.frombuffer(bytes(blob), dtype=np.uint8)
        mids = getattr(srcs, "mids", None) if mids is None else mids
        srcs = np.ascontiguousarray(srcs, dtype=SRC_DTYPE)
        jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
        tin = None if tails_in is None else np.ascontiguousarray(tails_in, dtype=np.int16)
        h = ctypes.c_void_p()
        if mids is not None and hasattr(self.L, "dcs_batch_create_mids"):
            mids = np.ascontiguousarray(mids, dtype=np.uint32)
            assert mids.shape == (srcs.size, 16)
            _check(self.L.dcs_batch_create_mids(ctx.h, _ptr(blob_a), blob_a.size, _ptr(srcs), _ptr(mids), srcs.size, _ptr(jobs), jobs.size,
                                                _ptr(tin), 0 if tin is None else tin.shape[0], ctypes.byref(h)), ctx.h)
        else:
            _check(self.L.dcs_batch_create(ctx.h, _ptr(blob_a), blob_a.size, _ptr(srcs), srcs.size, _ptr(jobs), jobs.size,
                                           _ptr(tin), 0 if tin is None else tin.shape[0], ctypes.byref(h)), ctx.h)
        self.h = h
        self.n_jobs = jobs.size
        ctx._batches.add(self)

    def run(self, stream=None):
        _check(self.L.dcs_batch_run(self.h, ctypes.c_void_p(stream) if stream else None), self.ctx.h)

    def run_many(self, count, stream=None):
        _check(self.L.dcs_batch_run_many(self.h, ctypes.c_void_p(stream) if stream else None, int(count)), self.ctx.h)

    def time(self, iters, stream=None):
        ms = ctypes.c_float(0)
        _check(self.L.dcs_batch_time(self.h, ctypes.c_void_p(stream) if stream else None, iters, ctypes.byref(ms)),
               self.ctx.h)
        return ms.value

    @staticmethod
    def time_rotating(batches, iters, stream=None):
        """average kernel time of `iters` launches dealt round-robin to `batches` (dcs_batch_time_rotating)"""
        b0 = batches[0]
        hs = (ctypes.c_void_p * len(batches))(*[b.h for b in batches])
        ms = ctypes.c_float(0)
        _check(b0.L.dcs_batch_time_rotating(hs, len(batches), ctypes.c_void_p(stream) if stream else None, iters, ctypes.byref(ms)), b0.ctx.h)
        return ms.value

    def sync(self):
        _check(self.L.dcs_batch_sync(self.h), self.ctx.h)

    def download(self, want_tails=False):
        pcm = np.zeros((self.n_jobs, FRAME_SAMPLES), dtype=np.int16)
        err = np.zeros(self.n_jobs, dtype=np.uint32)
        tails = np.zeros((self.n_jobs, 16), dtype=np.int16) if want_tails else None
        _check(self.L.dcs_batch_download(self.h, _ptr(pcm), _ptr(err), _ptr(tails)), self.ctx.h)
        return (pcm, err, tails) if want_tails else (pcm, err)

    def download_view(self):
        """PCM and error words as numpy views of the batch's pinned host memory (no copy into Python memory);
        valid until the batch is run again or closed"""
        p, e = ctypes.c_void_p(), ctypes.c_void_p()
        _check(self.L.dcs_batch_download_view(self.h, ctypes.byref(p), ctypes.byref(e)), self.ctx.h)
        pcm = _view(p, ctypes.c_int16, np.int16, (self.n_jobs, FRAME_SAMPLES))
        err = _view(e, ctypes.c_uint32, np.uint32, (self.n_jobs,))
        return pcm, err

    @property
    def algorithmic_bytes(self):
        return int(self.L.dcs_batch_algorithmic_bytes(self.h))

    @property
    def abi_bytes(self):
        return int(self.L.dcs_batch_abi_bytes(self.h))

    @property
    def num_chunks(self):
        return int(self.L.dcs_batch_num_chunks(self.h))

    @property
    def package_bytes(self):
        """bytes of one chunk package of this batch (the kernel reads num_chunks of them)"""
        return int(self.L.dcs_batch_package_bytes(self.h))

    @property
    def frames_per_wave(self):
        return int(self.L.dcs_batch_frames_per_wave(self.h))

    @property
    def even_deal(self):
        """the batch's packages deal 1994+ frames in units of 8 samples (Context.set_even_deal)"""
        return bool(self.L.dcs_batch_even_deal(self.h))

    @property
    def sole_source_kernel(self):
        """the batch's next launch runs the even-deal kernel without the rounds of further sources (Context.set_sole_source_kernel)"""
        return bool(self.L.dcs_batch_sole_source_kernel(self.h))

    @property
    def filled_bands(self):
        """the most header bands a source of the batch fills tile words for, as the kernel of a single-source even-deal batch is
        told (9: that or fewer; 16: also a batch that does not qualify)"""
        return int(self.L.dcs_batch_filled_bands(self.h))

    @property
    def chunks_per_wave(self):
        """chunks per wavefront of the batch's next launch (1 or 2; Decoder.set_chunks_per_wave)"""
        return int(self.L.dcs_batch_chunks_per_wave(self.h))

    def close(self):
        if self.h:
            if self.ctx.h:                      # (a closed context has already destroyed its batches)
                self.L.dcs_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Pipeline:
    """DcsPipeline: lists of whole streams in, PCM out in submission order, `depth` lists in flight.  flac=True: the lists
    leave the device as FLAC at 31 250 Hz (with the samples' MD5 if md5) and are collected with collect_flac()"""

    def __init__(self, ctx, depth=3, index_on_device=False, pack_on_device=False, plan_on_device=False, flac=False, md5=True):
        self.ctx = ctx
        self.L = ctx.L
        h = ctypes.c_void_p()
        flags = (1 if index_on_device else 0) | (2 if pack_on_device else 0) | (4 if plan_on_device else 0)
        flags |= (PIPE_FLAC | (PIPE_FLAC_MD5 if md5 else 0)) if flac else 0
        _check(self.L.dcs_pipeline_create(ctx.h, depth, flags, ctypes.byref(h)), ctx.h)
        self.h = h
        self._keep = []                         # (refs, byte buffers) of submitted lists, oldest first
        ctx._batches.add(self)                  # closed before the context, like a batch

    def submit_refs(self, refs, n, extra_frames=0, keep=None):
        """submit a prepared StreamRef array (see make_refs); the caller keeps it alive until collected"""
        self._keep.append((refs, keep))
        _check(self.L.dcs_pipeline_submit(self.h, refs, n, extra_frames), self.ctx.h)

    def submit(self, streams, extra_frames=0):
        streams = list(streams)
        refs, keep = _stream_refs(streams)
        self.submit_refs(refs, len(streams), extra_frames, keep)

    def collect(self):
        """-> (pcm [frames, 240], err, first frame of each stream, hostMs, deviceMs): views of pinned memory, valid
        until the next collect.  self.last_path: the stages of that list that ran on the device (bit 0 index walk, bit 1
        packer, bit 2 planner)"""
        r = PipelineResult()
        st = self.L.dcs_pipeline_collect(self.h, ctypes.byref(r))
        self.last_path = int(r.path)
        if self._keep and st != ERR_INVALID_ARG:        # (refused: the list is still the pipeline's, and its streams stay)
            self._keep.pop(0)
        _check(st, self.ctx.h)
        pcm = _view(r.pcm, ctypes.c_int16, np.int16, (r.nFrames, FRAME_SAMPLES))
        err = _view(r.err, ctypes.c_uint32, np.uint32, (r.nFrames,))
        first = _view(r.frameOffsets, ctypes.c_uint32, np.uint32, (r.nStreams + 1,))
        return pcm, err, first, r.hostMs, r.deviceMs

    def collect_flac(self):
        """a FLAC pipeline's collect -> (list of FLAC streams as bytes, FLAC_WRITE_INFO_DTYPE array, err, first frame of each
        stream, hostMs, deviceMs): copies of the pipeline's pinned memory.  self.last_path as collect() sets it"""
        r = PipelineFlacResult()
        st = self.L.dcs_pipeline_collect_flac(self.h, ctypes.byref(r))
        self.last_path = int(r.path)
        if self._keep and st != ERR_INVALID_ARG:
            self._keep.pop(0)
        _check(st, self.ctx.h)
        n = int(r.nStreams)
        offs = _view(r.flacOffsets, ctypes.c_uint64, np.uint64, (n + 1,))
        flac = _view(r.flac, ctypes.c_uint8, np.uint8, (int(offs[n]),))
        out = [flac[int(offs[k]):int(offs[k + 1])].tobytes() for k in range(n)]
        info = np.frombuffer(ctypes.string_at(r.info, FLAC_WRITE_INFO_DTYPE.itemsize * n), FLAC_WRITE_INFO_DTYPE).copy()
        err = _view(r.err, ctypes.c_uint32, np.uint32, (r.nFrames,)).copy()
        first = _view(r.frameOffsets, ctypes.c_uint32, np.uint32, (n + 1,)).copy()
        return out, info, err, first, r.hostMs, r.deviceMs

    def close(self):
        if self.h:
            if self.ctx.h:
                self.L.dcs_pipeline_destroy(self.h)
            self.h = None
            self._keep = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DevicePath:
    """DcsDevicePath: a list of whole streams resident in HBM; index walk, planner, packer and decode kernels run back to
    back on the device with nothing crossing PCIe (include/dcs_hip.h dcs_device_path_*)"""

    def __init__(self, ctx, streams, extra_frames=0):
        self.ctx = ctx
        self.L = ctx.L
        streams = list(streams)
        refs, keep = _stream_refs(streams)
        h = ctypes.c_void_p()
        _check(self.L.dcs_device_path_create(ctx.h, refs, len(streams), extra_frames, ctypes.byref(h)), ctx.h)
        self.h = h
        self.n_streams = len(streams)
        self.n_frames = int(sum(((int(k[0]) << 8) | int(k[1])) + extra_frames for k in keep))
        ctx._batches.add(self)                  # closed before the context, like a batch

    def run(self, iters=10):
        """-> dict of the DcsDevicePathTimes fields: ms per pass and per kernel"""
        t = DevicePathTimes()
        _check(self.L.dcs_device_path_run(self.h, int(iters), ctypes.byref(t)), self.ctx.h)
        return {f[0]: getattr(t, f[0]) for f in DevicePathTimes._fields_}

    def run_many(self, iters):
        """`iters` passes back to back and a wait; nothing timed"""
        _check(self.L.dcs_device_path_run_many(self.h, int(iters)), self.ctx.h)

    def download(self):
        pcm = np.zeros((self.n_frames, FRAME_SAMPLES), dtype=np.int16)
        err = np.zeros(self.n_frames, dtype=np.uint32)
        first = np.zeros(self.n_streams + 1, dtype=np.uint32)
        _check(self.L.dcs_device_path_download(self.h, _ptr(pcm), _ptr(err), _ptr(first)), self.ctx.h)
        return pcm, err, first

    def close(self):
        if self.h:
            if self.ctx.h:
                self.L.dcs_device_path_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Node:
    """DcsNode: several GPUs of one node behind one object -- persistent contexts, one pipeline each, lists dealt to the
    least-loaded device, results in submission order (include/dcs_hip.h dcs_node_*)"""

    def __init__(self, device_ids, depth=8, index_on_device=True, pack_on_device=True, plan_on_device=True):
        self.L = load_library()
        devs = np.ascontiguousarray(device_ids, dtype=np.int32)
        flags = (1 if index_on_device else 0) | (2 if pack_on_device else 0) | (4 if plan_on_device else 0)
        h = ctypes.c_void_p()
        st = self.L.dcs_node_create(_ptr(devs), devs.size, depth, flags, ctypes.byref(h))
        if st != 0:
            raise DcsError(st, "dcs_node_create")
        self.h = h
        self.n_devices = int(devs.size)
        self._keep = []

    def _check(self, st):
        if st != 0:
            raise DcsError(st, self.L.dcs_node_last_error(self.h).decode(errors="replace"))

    def submit_refs(self, refs, n, extra_frames=0, keep=None):
        self._keep.append((refs, keep))
        self._check(self.L.dcs_node_submit(self.h, refs, n, extra_frames))

    def submit(self, streams, extra_frames=0):
        streams = list(streams)
        refs, keep = _stream_refs(streams)
        self.submit_refs(refs, len(streams), extra_frames, keep)

    def collect(self):
        """-> (pcm, err, first frame of each stream, hostMs, deviceMs, index of the device that decoded the list)"""
        r = PipelineResult()
        dev = ctypes.c_int(-1)
        st = self.L.dcs_node_collect(self.h, ctypes.byref(r), ctypes.byref(dev))
        if self._keep:
            self._keep.pop(0)
        self._check(st)
        self.last_path = int(r.path)
        pcm = _view(r.pcm, ctypes.c_int16, np.int16, (r.nFrames, FRAME_SAMPLES))
        err = _view(r.err, ctypes.c_uint32, np.uint32, (r.nFrames,))
        first = _view(r.frameOffsets, ctypes.c_uint32, np.uint32, (r.nStreams + 1,))
        return pcm, err, first, r.hostMs, r.deviceMs, dev.value

    def device_info(self, index):
        """-> (HIP device id, NUMA node or -1, lists decoded so far)"""
        d, nn, done = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_uint64(0)
        self._check(self.L.dcs_node_device_info(self.h, index, ctypes.byref(d), ctypes.byref(nn), ctypes.byref(done)))
        return d.value, nn.value, done.value

    def close(self):
        if self.h:
            self.L.dcs_node_destroy(self.h)
            self.h = None
            self._keep = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_numa_node(device):
    """NUMA node of a HIP device (dcs_device_numa_node: from its PCI address), or -1"""
    return int(load_library().dcs_device_numa_node(int(device)))


def bind_process_to_device_numa(device):
    """bind the calling process (the threads it starts later inherit the mask, and the memory they pin or first touch is taken
    from that node under the default local policy) to the CPUs of the GPU's NUMA node; -> the node, or None when it is unknown
    or none of its CPUs may be used.  What dcs_node does per context, for a process that owns ONE GPU (a rank of bench.py)."""
    node = device_numa_node(device)
    if node < 0:
        return None
    try:
        text = open("/sys/devices/system/node/node%d/cpulist" % node).read().strip()
    except OSError:
        return None
    cpus = set()
    for part in text.split(","):
        if part:
            a, _, b = part.partition("-")
            cpus.update(range(int(a), int(b or a) + 1))
    allowed = cpus & os.sched_getaffinity(0)
    if not allowed:
        return None
    os.sched_setaffinity(0, allowed)
    return node


def node_cache_release():
    """destroy the contexts dcs_decode_streams_sharded keeps per device list"""
    load_library().dcs_node_cache_release()


def make_refs(streams):
    """StreamRef array for (os, bytes, volume, level) streams -> (refs, keep-alive buffers)"""
    return _stream_refs(list(streams))


class RomSet:
    """DcsRomSet: sound ROM images -> catalog, track programs, streams (include/dcs_hip.h, csrc/dcs_rom.cpp)"""

    def __init__(self, images=None, zip_path=None, zip_bytes=None, zip_name="roms.zip", explicit_u2=None):
        self.L = load_library()
        self.h = ctypes.c_void_p(self.L.dcs_romset_create())
        st = 0
        if images:
            for chip, data in images.items():
                st = st or self.L.dcs_romset_add_rom(self.h, chip, bytes(data), len(data))
        elif zip_path is not None:
            st = self.L.dcs_romset_load_zip(self.h, str(zip_path).encode(), explicit_u2.encode() if explicit_u2 else None)
        elif zip_bytes is not None:
            st = self.L.dcs_romset_load_zip_memory(self.h, zip_bytes, len(zip_bytes), zip_name.encode(),
                                                   explicit_u2.encode() if explicit_u2 else None)
        if st != 0:
            msg = self.L.dcs_romset_last_error(self.h).decode()
            self.close()
            raise DcsError(st, msg)

    def close(self):
        if self.h:
            self.L.dcs_romset_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self):
        c = RomCheck()
        _rs_check(self.L.dcs_romset_check(self.h, ctypes.byref(c)), self)
        return c

    def set_version(self, hw, os_):
        _rs_check(self.L.dcs_romset_set_version(self.h, hw, os_), self)

    @property
    def num_tracks(self):
        return self.L.dcs_romset_num_tracks(self.h)

    def track_info(self, track):
        ti = TrackInfo()
        return ti if self.L.dcs_romset_track_info(self.h, track, ctypes.byref(ti)) == 0 else None

    def decompile(self, track):
        n = ctypes.c_uint32()
        _rs_check(self.L.dcs_romset_decompile(self.h, track, None, 0, ctypes.byref(n)), self)
        ops = np.zeros(max(n.value, 1), dtype=TRACKOP_DTYPE)
        _rs_check(self.L.dcs_romset_decompile(self.h, track, _ptr(ops), n.value, ctypes.byref(n)), self)
        return ops[:n.value]

    def list_streams(self):
        n = ctypes.c_uint32()
        _rs_check(self.L.dcs_romset_list_streams(self.h, None, 0, ctypes.byref(n)), self)
        a = np.zeros(max(n.value, 1), dtype=np.uint32)
        _rs_check(self.L.dcs_romset_list_streams(self.h, _ptr(a), n.value, ctypes.byref(n)), self)
        return a[:n.value]

    def pointer(self, linear):
        """-> (chip number 2..9, offset in that chip's image, bytes available from there, address)"""
        p, avail, chip = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_int()
        _rs_check(self.L.dcs_romset_pointer(self.h, linear, ctypes.byref(p), ctypes.byref(avail), ctypes.byref(chip)), self)
        return chip.value, p.value, avail.value

    def stream_bytes(self, linear):
        _, p, avail = self.pointer(linear)
        return ctypes.string_at(p, avail)

    def extract_plan(self):
        n = ctypes.c_uint32()
        _rs_check(self.L.dcs_romset_extract_plan(self.h, None, 0, ctypes.byref(n)), self)
        a = np.zeros(max(n.value, 1), dtype=EXTRACT_DTYPE)
        _rs_check(self.L.dcs_romset_extract_plan(self.h, _ptr(a), n.value, ctypes.byref(n)), self)
        return a[:n.value]

    def extract_tracks_plan(self):
        """dcs_romset_extract_tracks_plan: [(track, frames of its WAV file)] of the --extract-tracks loop"""
        n = ctypes.c_uint32()
        _rs_check(self.L.dcs_romset_extract_tracks_plan(self.h, None, 0, ctypes.byref(n)), self)
        a = np.zeros((max(n.value, 1), 2), dtype=np.uint32)
        _rs_check(self.L.dcs_romset_extract_tracks_plan(self.h, _ptr(a), n.value, ctypes.byref(n)), self)
        return [(int(t), int(f)) for t, f in a[:n.value]]

    def add_rom(self, chip, data):
        _rs_check(self.L.dcs_romset_add_rom(self.h, chip, bytes(data), len(data)), self)

    def stream_refs(self, items, volume):
        refs = (StreamRef * max(len(items), 1))()
        items = np.ascontiguousarray(items, dtype=EXTRACT_DTYPE)
        _rs_check(self.L.dcs_romset_stream_refs(self.h, _ptr(items), len(items), volume, refs), self)
        return refs

    def dump(self, force_hw=-1, force_os=-1):
        """everything derived from the images as text, one item per line (the tests compare it with the same dump
        made from the reference's answers)"""
        c = self.check()
        out = ["check status=%d hw=%d os=%d nominal=%04x catalog=%x ntracks=%u sig=%s" % (
            c.status, c.hw, c.os, c.nominalVersion, c.catalogOffset, c.nTracks, c.signature.decode())]
        if force_hw >= 0 or force_os >= 0:
            self.set_version(force_hw if force_hw >= 0 else c.hw, force_os if force_os >= 0 else c.os)
        for t in range(self.num_tracks):
            ti = self.track_info(t)
            if ti is None:
                continue
            out.append("track %u addr=%06x ch=%d type=%d defer=%04x time=%u loop=%d" % (
                t, ti.address, ti.channel, ti.type, ti.deferCode & 0xFFFF, ti.time, ti.looping))
            if ti.type != 1:
                continue
            for op in self.decompile(t):
                out.append(" op off=%d nest=%d parent=%d delay=%04x opc=%02x n=%d bytes=%s" % (
                    op["offset"], op["nestingLevel"], op["loopParent"], op["delayCount"], op["opcode"], op["nOperandBytes"],
                    bytes(op["operandBytes"][:min(int(op["nOperandBytes"]), 8)]).hex()))
        base = {}
        for a in self.list_streams():
            chip, p, avail = self.pointer(int(a))
            if chip not in base:
                base[chip] = self.pointer((chip - 2) << (21 if self.check_hw() == HW_DCS95 else 20))[1]
            out.append("stream %06x chip=%d off=%x" % (a, chip, p - base[chip]))
        for it in self.extract_plan():
            out.append("extract track=%u num=%d addr=%06x level=%d" % (it["track"], it["streamNum"], it["address"], it["level"]))
        return "\n".join(out) + "\n"

    def check_hw(self):
        # the version in effect (after a possible override) shows in how a pointer is split
        chip, _, _ = self.pointer(1 << 20)
        return HW_DCS93 if chip == 3 else HW_DCS95


def _rs_check(st, rs):
    if st != 0:
        raise DcsError(st, rs.L.dcs_romset_last_error(rs.h).decode())


class Sequencer:
    """DcsSequencer: the track-program VM in front of the frame decode (csrc/dcs_sequencer.cpp)"""

    def __init__(self, romset, volume=255):
        self.L = load_library()
        self.rs = romset                        # keep the ROM set alive
        self.h = ctypes.c_void_p(self.L.dcs_seq_create(romset.h))
        if not self.h:
            raise DcsError(ERR_INVALID_ARG, "dcs_seq_create: ROM set without U2 or without versions")
        self.L.dcs_seq_set_master_volume(self.h, volume)

    def close(self):
        if self.h:
            self.L.dcs_seq_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def event(self, kind, value):
        """kind 0 data-port byte, 1 track command, 2 master volume, 3 ClearTracks"""
        if kind == 0: self.L.dcs_seq_write_data_port(self.h, value)
        elif kind == 1: self.L.dcs_seq_add_track_command(self.h, value)
        elif kind == 2: self.L.dcs_seq_set_master_volume(self.h, value)
        elif kind == 3: self.L.dcs_seq_clear_tracks(self.h)

    def set_rewindable(self, on=True):
        st = self.L.dcs_seq_set_rewindable(self.h, 1 if on else 0)
        if st != 0:
            raise DcsError(st)

    def rewind(self, keep_ticks):
        st = self.L.dcs_seq_rewind(self.h, keep_ticks)
        if st != 0:
            raise DcsError(st)

    def run_script(self, n_ticks, events):
        """plan n_ticks ticks, applying the (tick, kind, value) events before their tick"""
        e = 0
        events = sorted(events, key=lambda x: x[0])
        for t in range(n_ticks):
            while e < len(events) and events[e][0] <= t:
                self.event(events[e][1], events[e][2])
                e += 1
            st = self.L.dcs_seq_plan(self.h, 1)
            if st != 0:
                raise DcsError(st, self.L.dcs_seq_last_error(self.h).decode())

    def plan(self, n_ticks):
        st = self.L.dcs_seq_plan(self.h, n_ticks)
        if st != 0:
            raise DcsError(st, self.L.dcs_seq_last_error(self.h).decode())

    def plan_ahead(self, max_ticks, idle_ticks=2):
        """dcs_seq_plan_ahead -> ticks planned"""
        n = ctypes.c_uint32()
        st = self.L.dcs_seq_plan_ahead(self.h, max_ticks, idle_ticks, ctypes.byref(n))
        if st != 0:
            raise DcsError(st, self.L.dcs_seq_last_error(self.h).decode())
        return n.value

    def stream_playing_at(self, ticks, channel):
        return bool(self.L.dcs_seq_stream_playing_at(self.h, ticks, channel))

    def tracks_active_at(self, ticks):
        return bool(self.L.dcs_seq_tracks_active_at(self.h, ticks))

    def stream_playing(self, channel):
        return bool(self.L.dcs_seq_stream_playing(self.h, channel))

    def decode_view(self, ctx):
        """dcs_seq_decode_view: (pcm, err) copied out of the context's pinned memory"""
        pcm, err, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint32()
        _check(self.L.dcs_seq_decode_view(ctx.h, self.h, ctypes.byref(pcm), ctypes.byref(n), ctypes.byref(err)), ctx.h)
        if n.value == 0:
            return np.zeros((0, FRAME_SAMPLES), dtype=np.int16), np.zeros(0, dtype=np.uint32)
        p = np.frombuffer(ctypes.string_at(pcm.value, n.value * FRAME_SAMPLES * 2), dtype=np.int16).reshape(n.value, FRAME_SAMPLES).copy()
        e = np.frombuffer(ctypes.string_at(err.value, n.value * 4), dtype=np.uint32).copy()
        return p, e

    @property
    def pending_ticks(self):
        return self.L.dcs_seq_pending_ticks(self.h)

    @property
    def fatal(self):
        return bool(self.L.dcs_seq_is_fatal(self.h))

    def host_bytes(self):
        n = self.L.dcs_seq_host_bytes(self.h, None, 0)
        a = np.zeros((max(n, 1), 2), dtype=np.uint32)
        self.L.dcs_seq_host_bytes(self.h, _ptr(a), n)
        return [(int(t), int(b)) for t, b in a[:n]]

    def decode(self, ctx):
        n = self.pending_ticks
        pcm = np.zeros((n, FRAME_SAMPLES), dtype=np.int16)
        err = np.zeros(max(n, 1), dtype=np.uint32)
        _check(self.L.dcs_seq_decode(ctx.h, self.h, _ptr(pcm), n, _ptr(err)), ctx.h)
        return pcm, err[:n]
