"""Budgets from any source without a GPU: dcs_transcode_plan_budget against the restated copy rule, the refusals the budget
calls make before they touch a device, the header, and the restated chain's own claims on the small lists the GPU tests run
(tests/budget_chain_ref.py), pinned in tests/golden/budget_chain_golden.json."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import budget_chain_ref as B
import enc94rd_cases as C94
import dcsexplorer_amd as D
import dcsexplorer_amd.api as A
import transcode_ref as T
from dcsexplorer_amd.api import StreamRef
from util import make_stream

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "budget_chain_golden.json")))
RATE = 32000


def _fmt(version):
    return D.FMT_94_T0 if version == 0x9400 else None


def _srcs():
    return [(make_stream(fmt, 5 + fmt, seed=0x90 + fmt), D.format_os(fmt)) for fmt in range(6)]


# ---------------------------------------------------------------------------------------------------------------- the plan

@pytest.mark.parametrize("version", B.VERSIONS, ids=lambda v: "%x" % v)
def test_plan_follows_the_copy_rule(version):
    srcs = _srcs()
    streams, oss = [s for s, _ in srcs], [o for _, o in srcs]
    lens = [len(s) for s in streams]
    copyable = [T.action(s, o, version) == T.COPIED for s, o in srcs]
    assert any(copyable) and not all(copyable)
    rd_bound = D.encode_rd_bound if version == 0x9400 else D.encode93_rd_bound
    forms = [dict(), dict(reencode_all=True)]
    for delta in (0, -1, 1):
        bounds = [n + delta for n in lens]
        forms += [dict(budget=bounds), dict(total=10 ** 6, cap=bounds), dict(budget=bounds, reencode_all=True)]
    forms += [dict(total=0), dict(total=10 ** 6)]
    for kw in forms:
        action, bound = D.transcode_plan_budget(streams, oss, version, _fmt(version), **kw)
        want = [B.copied(copyable[j], lens[j], j, kw.get("budget"), kw.get("total"), kw.get("cap"), kw.get("reencode_all", False))
                for j in range(6)]
        assert [int(a) == T.COPIED for a in action] == want, kw
        assert [int(b) for b in bound] == [lens[j] if want[j] else rd_bound((T.frames(streams[j]) + 1) * 240) for j in range(6)], kw
    # equal to the bound copies, one below it searches, one above it copies
    j = copyable.index(True)
    for delta, copies in ((0, True), (-1, False), (1, True)):
        b = [10 ** 6] * 6
        b[j] = lens[j] + delta
        assert (int(D.transcode_plan_budget(streams, oss, version, _fmt(version), budget=b)[0][j]) == T.COPIED) == copies
        assert (int(D.transcode_plan_budget(streams, oss, version, _fmt(version), total=5, cap=b)[0][j]) == T.COPIED) == copies


# ----------------------------------------------------------------------------------------------------------- the refusals

def _budget(**kw):
    return D.Budget(kw.get("budgetBytes"), kw.get("totalBytes", 0), kw.get("capBytes"), kw.get("shared", 0), None)


def test_refusals_before_any_device_work():
    L = D.load_library()
    s, os_ = _srcs()[3]
    keep = np.frombuffer(s, np.uint8)
    ref = StreamRef()
    ref.data, ref.len, ref.os, ref.volume, ref.level, ref.channelVolume = keep.ctypes.data, len(s), os_, 0x67, 0xFF, 0xFF
    action, bound = np.zeros(1, np.int32), np.zeros(1, np.uint64)
    good = D.transcode_params(0x9302)
    plan = lambda p, b: L.dcs_transcode_plan_budget(ctypes.byref(ref), 1, ctypes.byref(p) if p is not None else None, 0,
                                                    ctypes.byref(b) if b is not None else None, action.ctypes.data, bound.ctypes.data)
    assert plan(good, _budget()) == 0
    # an OS93 Type 1 target, either version
    assert plan(D.transcode_params(0x9301, D.FMT_93A_T1), _budget()) == A.ERR_INVALID_ARG
    t1 = D.transcode_params(0x9302)
    t1.streamFormatType = 1
    assert plan(t1, _budget()) == A.ERR_INVALID_ARG
    # shared with budgetBytes set; a shared value that is neither form; null arguments
    bud = np.asarray([500], np.uint32)
    assert plan(good, _budget(budgetBytes=bud.ctypes.data, shared=1, totalBytes=900)) == A.ERR_INVALID_ARG
    assert plan(good, _budget(shared=2)) == A.ERR_INVALID_ARG
    assert plan(good, None) == A.ERR_INVALID_ARG and plan(None, _budget()) == A.ERR_INVALID_ARG
    assert L.dcs_transcode_plan_budget(None, 1, ctypes.byref(good), 0, ctypes.byref(_budget()), None, None) == A.ERR_INVALID_ARG
    assert L.dcs_transcode_plan_budget(ctypes.byref(ref), 1, ctypes.byref(good), 2, ctypes.byref(_budget()), None, None) == A.ERR_INVALID_ARG
    # the calls that take a context refuse a null one, a null budget and null offsets before anything else
    b, offs = _budget(), np.zeros(2, np.uint64)
    assert L.dcs_transcode_streams_budget(None, ctypes.byref(ref), 1, ctypes.byref(good), 0, ctypes.byref(b), None, 0, offs.ctypes.data,
                                          None, None) == A.ERR_INVALID_ARG
    assert L.dcs_encode_streams_at_budget(None, None, offs.ctypes.data, 0, None, None, None, 0, ctypes.byref(good), ctypes.byref(b), None, 0,
                                          offs.ctypes.data, None, None, None, 0, None) == A.ERR_INVALID_ARG
    assert L.dcs_encode_files_budget(None, None, offs.ctypes.data, 0, ctypes.byref(good), None, 0, ctypes.byref(b), None, 0,
                                     offs.ctypes.data, None, None, None, 0, None) == A.ERR_INVALID_ARG
    # a stream too short to have a type bit is a bad stream, as in dcs_transcode_plan
    ref.len = 2
    assert plan(good, _budget()) == A.ERR_BAD_STREAM
    # a bad file, in the files call's host-only plan: what dcs_encode_files_plan says of the same list (the messages, which
    # need a context, are the GPU test's)
    files = list(B.mixed_files(0x9302))
    kinds, bounds = np.zeros(5, np.int32), np.zeros(5, np.uint64)
    def files_plan(fs, b, flags=0):
        blob = np.frombuffer(b"".join(fs), np.uint8)
        fo = np.cumsum([0] + [len(f) for f in fs]).astype(np.uint64)
        return (L.dcs_encode_files_plan_budget(blob.ctypes.data, fo.ctypes.data, len(fs), ctypes.byref(good), None, flags, ctypes.byref(b),
                                               kinds.ctypes.data, bounds.ctypes.data),
                L.dcs_encode_files_plan(blob.ctypes.data, fo.ctypes.data, len(fs), ctypes.byref(good), None, flags & 1, None, None, None))
    assert files_plan(files, _budget()) == (0, 0)
    assert [int(k) for k in kinds] == [A.FILE_WAV, A.FILE_DCSA_REENCODE, A.FILE_FLAC, A.FILE_DCSA_COPY, A.FILE_WAV]
    own = len(D.dcsa_parse(files[3])[1])
    assert int(bounds[3]) == own and all(int(v) >= D.encode93_rd_bound(240) for k, v in enumerate(bounds) if k != 3)
    assert files_plan(files, _budget(), A.FILES_REENCODE_ALL)[0] == 0 and int(kinds[3]) == A.FILE_DCSA_REENCODE and int(bounds[3]) > own
    for bad_file in (files[0][:30], b"fLaC" + bytes(40), b"neither of them"):
        got, want = files_plan([files[4], bad_file, files[0]], _budget())
        assert got == want != 0
    assert files_plan(files, _budget(budgetBytes=bud.ctypes.data, shared=1))[0] == A.ERR_INVALID_ARG


# -------------------------------------------------------------------------------------------------------------- the header

def test_header_struct_and_abi_sentence():
    hdr = open(os.path.join(HERE, "..", "include", "dcs_hip.h")).read()
    body = re.search(r"typedef struct DcsBudget\s*\{(.*?)\}\s*DcsBudget;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(const uint32_t \*|uint64_t|uint32_t|DcsEncodeRdFitInfo \*)\s*(\w+);", body, re.M)
    assert [f[1] for f in fields] == ["budgetBytes", "totalBytes", "capBytes", "shared", "fit"] == [f[0] for f in D.Budget._fields_]
    at = 0
    for (ctype, name), (_, py) in zip(fields, D.Budget._fields_):
        size = 4 if ctype == "uint32_t" else 8
        at = (at + size - 1) // size * size
        assert getattr(D.Budget, name).offset == at and ctypes.sizeof(py) == size, name
        at += size
    assert ctypes.sizeof(D.Budget) == (at + 7) // 8 * 8 == 40
    assert "DCS_ABI_VERSION stays 9" in hdr and "#define DCS_ABI_VERSION 9 " in hdr
    sentence = hdr[hdr.index("DCS_ABI_VERSION stays 9"):]
    for name in ("DcsBudget", "dcs_encode_streams_at_budget", "dcs_transcode_plan_budget", "dcs_transcode_streams_budget",
                 "dcs_encode_files_plan_budget", "dcs_encode_files_budget"):
        assert name in sentence[:400], name
        assert name in A.EXPORTS or name == "DcsBudget"
    assert D.load_library().dcs_abi_version() == 9


# ------------------------------------------------------------------------------------------- the restated chain's own claims

def _decodes_with(oracle, version, raw, an):
    """the oracle reads the stream to its last bit, and its frame buffers give the sqErr reported against the targets"""
    s, ch = raw[0], raw[1]
    F = T.frames(s)
    if version == 0x9400:
        R, os_, probe, m0 = B.R94, (D.OS95 if ch["sub"] == 3 else D.OS94), C94.closing_probe(s, ch, raw[3]), B.R94.M0
    else:
        R, os_, probe, m0 = B.R93, B.R93.OS_OF[version], s + bytes(8), B.R93.M0[version]
    assert len(s) == 18 + (ch["frameBits"] + 7) // 8 and F == an["t"].shape[0]
    out, offs, _, stops = oracle.decompress(os_, probe, m0, F + 1)
    assert not stops[:F].any()
    assert offs[F] - offs[0] == ch["frameBits"]
    fb = out[:F, :256].astype(np.int16).astype(np.int64)
    assert int(((R.frame_buffer(an["t"]) - fb) ** 2).sum()) == ch["sqErr"]


@pytest.mark.parametrize("version", B.VERSIONS, ids=lambda v: "%x" % v)
def test_restated_chain_on_the_mixed_list(oracle, version):
    files = B.mixed_files(version)
    units = B.file_units(oracle, files, version)
    assert [u[0] for u in units] == ["pcm", "pcm", "pcm", "copy", "pcm"]
    budgets = B.rate_budgets(units, RATE)
    total = sum(budgets)
    for key, kw in (("per-job", dict(budget=budgets)), ("shared", dict(total=total)), ("rate", dict())):
        streams, infos, rec, allot, raws = B.run(version, units, **kw)
        assert B.digest(streams, infos, rec) == GOLDEN["mixed"]["%x-%s" % (version, key)], key
        assert streams[3] == units[3][1] and infos[3] == B.COPY_INFO
        for j, (u, s, i) in enumerate(zip(units, streams, infos)):
            if u[0] == "pcm":
                assert raws[j][0][0] == s and raws[j][0][1]["sqErr"] == i[6]
                _decodes_with(oracle, version, *raws[j])
                if key == "per-job":
                    assert len(s) <= budgets[j] or not i[7]
        if rec is not None:
            # allotments plus copies stay within the total whenever it fits; a searched stream is as long as its allotment
            assert rec["fits"] == 1 and sum(allot) == rec["usedBytes"] <= total == rec["totalBytes"]
            assert [len(s) for s in streams] == allot
            # the shared form moves bytes: the near-silent file is below its rate share, the dense one above it
            assert allot[4] < budgets[4] and allot[0] > budgets[0]
    # the copies alone exceed the total: fits = 0, every searched job at its first vertex
    copies = len(units[3][1])
    streams, infos, rec, allot, _ = B.run(version, units, total=copies - 1)
    huge = B.run(version, units, total=10 ** 9)[2]
    assert rec["fits"] == 0 and rec["usedBytes"] == rec["leastBytes"] == huge["leastBytes"] > copies
    assert B.digest(streams, infos, rec) == GOLDEN["mixed"]["%x-exceeded" % version]
    # a cap below the copyable container's length has it searched
    cap = [10 ** 6] * 5
    cap[3] = copies - 1
    assert [u[0] for u in B.file_units(oracle, files, version, total=10 ** 6, cap=cap)] == ["pcm"] * 5
