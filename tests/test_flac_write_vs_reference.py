"""The FLAC writer's restatement (tests/flac_write_ref.py) against the compiled libFLAC on the seeded streams of
tests/flac_write_fuzz_cases.py, no GPU: FLAC__stream_decoder with MD5 checking (oracle/_ref/dcs_flacref md5) accepts every
file, written with and without the MD5, decodes it to the source, and the MD5 passes.  No exclusions.  The sets must make
every choice the writer has: the counts are asserted on the restatement here and printed."""
import pytest

import flac_fuzz_cases as Z
import flac_write_fuzz_cases as C
import flac_write_ref as R


def test_the_sets_make_every_choice():
    C.check_tally([s for items in C.sets().values() for s in items])


@pytest.mark.skipif(not Z.checker_available(), reason=Z.MISSING)
@pytest.mark.parametrize("md5", [True, False], ids=["md5", "nomd5"])
def test_libflac_decodes_every_stream_to_its_source(md5):
    streams = [s for items in C.sets().values() for s in items]
    verdicts = Z.check_md5([(R.write(x, 31250, md5)[0], x) for _, x in streams])
    failed = [(name, v) for (name, _), v in zip(streams, verdicts) if v != "ok"]
    assert len(verdicts) == len(streams) and not failed, failed
