"""The any-length FLAC writer's restatement (tests/flac_write_any_ref.py) against the compiled libFLAC on the seeded streams of
tests/flac_write_any_fuzz_cases.py, no GPU: FLAC__stream_decoder with MD5 checking (oracle/_ref/dcs_flacref md5) accepts
every file, written with and without the MD5, decodes it to the source, and the MD5 passes.  The input is well-formed PCM, so
no case is set aside.  The streams must make every choice the branch for last blocks with n & 15 != 0 has: the counts are
asserted on the restatement here and printed."""
import pytest

import flac_fuzz_cases as Z
import flac_write_any_fuzz_cases as C
import flac_write_any_ref as A


def test_the_streams_make_every_choice():
    t = C.check_tally()
    print("\n%d streams in %d families; choices over the last blocks with n & 15 != 0:\n%s" % (len(C.streams()), len(C.sets()), t))
    assert all(v >= 1 for v in t.values())
    assert {C.last_block(x).size for _, x in C.streams()} >= set(C.LENGTHS)


@pytest.mark.skipif(not Z.checker_available(), reason=Z.MISSING)
@pytest.mark.parametrize("md5", [True, False], ids=["md5", "nomd5"])
def test_libflac_decodes_every_stream_to_its_source(md5):
    streams = C.streams()
    verdicts = Z.check_md5([(A.write(x, C.RATE, md5)[0], x) for _, x in streams])
    failed = [(name, v) for (name, _), v in zip(streams, verdicts) if v != "ok"]
    print("\n%d streams, %d ok, 0 set aside" % (len(streams), len(verdicts) - len(failed)))
    assert len(verdicts) == len(streams) and not failed, failed[:20]
