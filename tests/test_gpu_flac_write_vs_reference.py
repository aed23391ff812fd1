"""The FLAC writer on the MI355X (dcs_flac_write_streams) against its numpy restatement, byte for byte, on the seeded streams
of tests/flac_write_fuzz_cases.py: content at the ties and thresholds of the writer's choices, every last-block length.  Each
set goes up in one call, then shuffled with one-frame fillers between its streams (other offsets, other block indices), then
a few streams alone.  tests/test_flac_write_vs_reference.py ties the restatement's files to the compiled libFLAC."""
import numpy as np
import pytest

import flac_write_fuzz_cases as C
import flac_write_ref as R
from dcsexplorer_amd.api import FLAC_WRITE_INFO_DTYPE

pytestmark = pytest.mark.gpu

SETS = list(C.sets())
FIELDS = FLAC_WRITE_INFO_DTYPE.names


@pytest.fixture(scope="module")
def ref():
    """the restatement's (bytes, info) of every stream and filler, with the MD5; computed once, never changed"""
    out = {name: R.write(x, 31250, True) for items in C.sets().values() for name, x in items}
    out.update({("filler", i): R.write(x, 31250, True) for i, x in enumerate(C.fillers())})
    return out


def check(ctx, names, pcm, ref, what):
    out, info = ctx.flac_write_streams(pcm)
    assert len(out) == len(names)
    for k, name in enumerate(names):
        want, want_info = ref[name]
        assert out[k] == want, (what, name, len(out[k]), len(want))
        assert {f: int(info[k][f]) for f in FIELDS} == want_info, (what, name)
    return out


@pytest.mark.parametrize("name", SETS)
def test_set_byte_for_byte_in_three_compositions(gpu_ctx, ref, name):
    items = C.sets()[name]
    out = check(gpu_ctx, [n for n, _ in items], [x for _, x in items], ref, "one call")
    # the library's own reader on the library's own files: int16 / 32767.f, bit for bit
    for (n, x), got in zip(items, gpu_ctx.flac_decode(out)):
        want = x.astype(np.float32) / np.float32(32767)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), n
    order, lead = C.shuffled(len(items), SETS.index(name))
    fill = C.fillers()
    names, pcm = [], []
    for i, k in zip(order, lead):
        for j in range(k):
            names.append(("filler", (i + j) % len(fill)))
            pcm.append(fill[(i + j) % len(fill)])
        names.append(items[i][0])
        pcm.append(items[i][1])
    check(gpu_ctx, names, pcm, ref, "shuffled with fillers")
    for i in order[:3]:
        check(gpu_ctx, [items[i][0]], [items[i][1]], ref, "alone")


def test_without_md5(gpu_ctx):
    items = [s for name in ("lengths", "full_scale") for s in C.sets()[name]]
    out, info = gpu_ctx.flac_write_streams([x for _, x in items], md5=False)
    for (n, x), got in zip(items, out):
        assert got == R.write(x, 31250, False)[0], n


def test_the_counts_the_sets_made(gpu_ctx):
    """the block kinds, fixed orders, partition orders and Rice parameters of all sets, by the restatement the GPU's bytes
    equal: every choice at least 20 times, every parameter 0 to 14 at least once (printed)"""
    C.check_tally([s for items in C.sets().values() for s in items])
