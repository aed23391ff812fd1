"""dcsexplorer_amd -- MI355X-native batched decoder for DCS pinball audio frames.

Python is only the thin test/bench harness over the C ABI of ``libdcs_hip.so``
(``include/dcs_hip.h``); the product is the shared library: host C++ (index pass, mixing
parameters, chunk planner, DCSDecoderHIP class) plus hand-written gfx950 HIP kernels.
"""
from .api import (  # noqa: F401
    OS93A, OS93B, OS94, OS95,
    FMT_93_T0, FMT_93B_T1, FMT_93A_T1, FMT_94_T0, FMT_94_T1_S0, FMT_94_T1_S3,
    FRAME_SAMPLES, FRAME_STOP, FRAME_FATAL, PREV_NONE, PREV_EXT, XFORM_93, XFORM_94,
    SRC_DTYPE, JOB_DTYPE, INDEX_DTYPE, IDX_SERIAL,
    DcsError, lib_path, load_library, build_id, lib_sha256,
    index_stream, index_stream_mids, even_deal_lane, index_streams, pack_streams, stream_params, volume_multiplier, mixing_multiplier, frame_scale,
    synth_stream, wav_header, dcsa_header, dcsa_parse, frame_diff, build_stream_batch, device_count, plan_chunks, pack_chunks, format_os,
    Context, Batch, RomSet, Sequencer, HW_DCS93, HW_DCS95,
    host_threads, partition_streams, decode_streams_sharded, Pipeline, make_refs, FRAME_TAIL_LOST, Node, DevicePath, node_cache_release, device_numa_node, bind_process_to_device_numa,
    FMT_94_T0_S3, ENCODE_INFO_DTYPE, EncodeParams, encode_params, encode_bound, encode_header,
    encode93_params, encode93_bound, encode93_header, ENCODE93A_INFO_DTYPE, encode93a_bound, ENCODE_RD_INFO_DTYPE, encode_rd_bound, encode93_rd_bound, encode93a_params,
    ENCODE_RD_FIT_INFO_DTYPE, encode_rd_allot,
    SWEEP_RESULT_DTYPE, SWEEP_JOB_DTYPE, SWEEP_MEASURE, sweep_sq_err, encode_sweep_group_frames, encode_fit_choose,
    TRANSCODE_COPIED, TRANSCODE_REENCODED, TRANSCODE_REENCODE_ALL, TRANSCODE_INFO_DTYPE, TRANSCODE_OS, transcode_params, transcode_plan, transcode_plan_budget, Budget, FILES_REENCODE_ALL,
    ResampleFilter, RESAMPLE_AT_UNITY, resample_filter_default, resample_count,
    OUT_SEQUENCE, RATE_INFO_DTYPE, resample_out_count, resample_out_walk,
    WavInfo, ENCODE_FILE_INFO_DTYPE, WAV_U8, WAV_S16, WAV_S24, WAV_S32, WAV_F32, WAV_F64, WAV_IMA, FILE_WAV, FILE_DCSA_COPY,
    FILE_DCSA_REENCODE, FILE_WALK_NONE, FILE_WALK_DEVICE, FILE_WALK_HOST, wav_parse, encode_files_plan,
    FlacInfo, FLAC_FRAME_DTYPE, WAV_S8, FILE_FLAC, flac_parse, flac_index,
    FLAC_MD5, FLAC_SEQUENCE, FLAC_WRITE_INFO_DTYPE, PIPE_FLAC, PIPE_FLAC_MD5, PipelineFlacResult, flac_write_bound, flac_write_check,
    FLAC_AT_UNITY, flac_write_samples_check,
    Level, LEVEL_GAIN, LEVEL_FIT, LEVEL_NORMALIZE, LEVEL_CLIP, LEVEL_INFO_DTYPE, level_gain,
)
