"""The any-length FLAC writer on the MI355X (dcs_flac_write_samples) on the seeded streams of
tests/flac_write_any_fuzz_cases.py: last blocks that are no multiple of 16 samples with content at the ties and thresholds
of the writer's choices.  Each family goes up in one call, then all families in one call, shuffled, with one-sample and
240-sample fillers between the streams (other offsets, odd and even, other block indices).  The bytes and the info fields
equal the restatement's (tests/flac_write_any_ref.py), and the library's own bytes pass the compiled libFLAC's decoder with
MD5 checking against the source PCM (oracle/_ref/dcs_flacref md5, where `build()` made it)."""
import numpy as np
import pytest

import flac_fuzz_cases as Z
import flac_write_any_fuzz_cases as C
import flac_write_any_ref as A
from dcsexplorer_amd.api import FLAC_WRITE_INFO_DTYPE

pytestmark = pytest.mark.gpu

FAMILIES = list(C.sets())
FIELDS = FLAC_WRITE_INFO_DTYPE.names


@pytest.fixture(scope="module")
def ref():
    """the restatement's (bytes, info) of every stream and filler, with the MD5; computed once, never changed"""
    out = {name: A.write(x, C.RATE, True) for name, x in C.streams()}
    out.update({("filler", i): A.write(x, C.RATE, True) for i, x in enumerate(C.fillers())})
    return out


def check(ctx, names, pcm, ref, what):
    out, info = ctx.flac_write_samples(pcm, C.RATE)
    assert len(out) == len(names)
    for k, name in enumerate(names):
        want, want_info = ref[name]
        assert out[k] == want, (what, name, len(out[k]), len(want))
        assert {f: int(info[k][f]) for f in FIELDS} == want_info, (what, name)
    return out


def check_libflac(out, pcm, names):
    if not Z.checker_available():
        return 0
    verdicts = Z.check_md5(list(zip(out, pcm)))
    failed = [(n, v) for n, v in zip(names, verdicts) if v != "ok"]
    assert len(verdicts) == len(out) and not failed, failed[:20]
    return len(verdicts)


@pytest.mark.parametrize("family", FAMILIES)
def test_family_byte_for_byte_and_through_libflac(gpu_ctx, ref, family):
    items = C.sets()[family]
    names, pcm = [n for n, _ in items], [x for _, x in items]
    out = check(gpu_ctx, names, pcm, ref, "one call")
    n = check_libflac(out, pcm, names)
    print("\n%s: %d streams equal the restatement, %d of the library's files pass libFLAC's MD5 check" % (family, len(out), n))


def test_all_families_shuffled_with_fillers(gpu_ctx, ref):
    items = C.streams()
    order, lead = C.shuffled(len(items))
    fill = C.fillers()
    names, pcm = [], []
    for i, k in zip(order, lead):
        for j in range(k):
            names.append(("filler", (i + j) % len(fill)))
            pcm.append(fill[(i + j) % len(fill)])
        names.append(items[i][0])
        pcm.append(items[i][1])
    starts = np.cumsum([0] + [x.size for x in pcm])[:-1]
    assert (starts % 2 == 1).sum() > 100 and (starts % 2 == 0).sum() > 100 and {x.size for x in fill} == {1, 240}
    out = check(gpu_ctx, names, pcm, ref, "shuffled with fillers")
    check_libflac(out, pcm, names)


def test_without_md5(gpu_ctx):
    items = [s for family in ("full_scale", "partition_steps", "binding") for s in C.sets()[family]]
    out, _ = gpu_ctx.flac_write_samples([x for _, x in items], C.RATE, md5=False)
    for (n, x), got in zip(items, out):
        assert got == A.write(x, C.RATE, False)[0], n
    check_libflac(out, [x for _, x in items], [n for n, _ in items])


def test_the_choices_the_streams_made():
    print("\nchoices over the last blocks with n & 15 != 0:", C.check_tally())
