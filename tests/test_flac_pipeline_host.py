"""FLAC as a pipeline output, the parts that need no GPU: DcsPipelineFlacResult's layout as the bindings state it, the new
constants, and the new entry point in the bindings' list and in the header (tests/test_abi.py then holds the library to it)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "dcs_hip.h")).read()


def test_result_struct_layout(dcs):
    R = dcs.PipelineFlacResult
    assert ctypes.sizeof(R) == 64
    want = dict(flac=0, flacOffsets=8, info=16, err=24, frameOffsets=32, nFrames=40, nStreams=44, status=48, hostMs=52, deviceMs=56, path=60)
    assert {name: getattr(R, name).offset for name, _ in R._fields_} == want
    assert "typedef struct DcsPipelineFlacResult" in header()
    # the PCM result is what it was
    assert ctypes.sizeof(dcs.api.PipelineResult) == 48


def test_constants(dcs):
    assert (dcs.PIPE_FLAC, dcs.PIPE_FLAC_MD5) == (8, 16)
    hdr = header()
    assert int(re.search(r"#define\s+DCS_PIPE_FLAC\s+(\d+)u", hdr).group(1)) == dcs.PIPE_FLAC
    assert int(re.search(r"#define\s+DCS_PIPE_FLAC_MD5\s+(\d+)u", hdr).group(1)) == dcs.PIPE_FLAC_MD5
    assert int(re.search(r"#define\s+DCS_ABI_VERSION\s+(\d+)", hdr).group(1)) == dcs.api.ABI_VERSION == 9


def test_entry_point_is_declared_bound_and_exported(dcs):
    assert "dcs_pipeline_collect_flac" in dcs.api.EXPORTS
    assert re.search(r"DcsStatus\s+dcs_pipeline_collect_flac\s*\(\s*DcsPipeline\s*\*\s*p\s*,\s*DcsPipelineFlacResult\s*\*\s*out\s*\)\s*;", header())
    L = dcs.load_library()
    assert L.dcs_pipeline_collect_flac.argtypes[1]._type_ is dcs.PipelineFlacResult
    assert L.dcs_pipeline_collect_flac(None, None) == dcs.api.ERR_INVALID_ARG
