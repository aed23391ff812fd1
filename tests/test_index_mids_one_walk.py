"""The mid records come from the index walk itself: what index_stream_mids returns is what the commit before that change
returned (tests/golden/mids_golden.json, made from that commit's library by tests/golden/make_mids_golden.py), its records and
summary are those of the walk without mid records, and the many-stream entry equals the per-stream one.  No GPU."""
import json
import os

import numpy as np
import pytest

import dcsexplorer_amd as D
import mids_cases as C

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mids_golden.json")))["cases"]

_INDEXED = None


def indexed():
    """-> [(records, StreamInfo, mids)] of index_stream_mids, per case, made once"""
    global _INDEXED
    if _INDEXED is None:
        _INDEXED = [D.index_stream_mids(os_, s) for _, os_, s in C.cases()]
    return _INDEXED


def test_hashes_are_the_parents():
    assert sorted(GOLDEN) == sorted(name for name, _, _ in C.cases())
    wrong = [name for (name, _, _), got in zip(C.cases(), indexed()) if C.digest(*got) != GOLDEN[name]]
    assert not wrong, wrong


def test_error_frames_and_1993_layouts_have_zero_mids():
    for (name, _, _), (idx, info, mids) in zip(C.cases(), indexed()):
        clean = (idx["flags"] == 0) & (info.format >= D.FMT_94_T0)
        assert not mids[~clean].any() and (mids[clean, 0] == 1).all(), name


def test_records_and_summary_equal_the_walks_without_mids():
    """the walk that records the middles takes the multi-code table in shorter runs: records, nBytes, payloadBits and
    nValidFrames must not move -- against the same walker without mid records and against the literal reader"""
    for (name, os_, s), (idx, info, _) in zip(C.cases(), indexed()):
        for literal in (False, True):
            idx2, info2 = D.index_stream(os_, s, literal=literal)
            assert idx.tobytes() == idx2.tobytes() and bytes(info) == bytes(info2), (name, literal)
            assert (info.nBytes, info.payloadBits, info.nValidFrames) == (info2.nBytes, info2.payloadBits, info2.nValidFrames)


@pytest.mark.parametrize("threads", [1, 2, 5])
def test_many_streams_equal_the_per_stream_call(threads):
    many = D.index_streams([(os_, s) for _, os_, s in C.cases()], threads=threads, with_mids=True)
    assert len(many) == len(indexed())
    for (name, _, _), (idx, info, mids), (idx2, info2, mids2) in zip(C.cases(), indexed(), many):
        assert idx.tobytes() == idx2.tobytes() and bytes(info) == bytes(info2) and np.array_equal(mids, mids2), name
