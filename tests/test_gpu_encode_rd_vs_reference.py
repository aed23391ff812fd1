"""The rate-distortion 1994+ encoder on the MI355X against the reference: the quality condition on the device's own bytes.
B and E are the length and the time-domain error (sweep_ref.measure on the library's own decode) of the reference-equal
stream, which is dcs_encode_streams' here; dcs_encode_rd_streams with budgetBytes = B writes at most B bytes with an error
of at most E, for four signals, the three layouts and the six rates of sweep_ref.RATES.  The bytes are the restatement's."""
import numpy as np
import pytest

import dcsexplorer_amd as D
import enc94rd_cases as C
import enc94rd_ref as R
import sweep_ref as S

pytestmark = pytest.mark.gpu

FMT = {(0, 0): D.FMT_94_T0, (1, 0): D.FMT_94_T1_S0, (1, 3): D.FMT_94_T1_S3}


def _errors(gpu_ctx, lay, x, streams):
    os_ = D.OS95 if lay[1] == 3 else D.OS94
    pcm, err, first = gpu_ctx.decode_streams([(os_, s, 255, 0xFF) for s in streams], extra_frames=1)
    assert not err.any()
    first = list(first) + [pcm.shape[0]]
    return [S.sq_err(S.measure(x, pcm[first[k]:first[k + 1]])) for k in range(len(streams))]


@pytest.mark.parametrize("name", C.QUALITY_GPU)
def test_quality_on_the_devices_own_bytes(gpu_ctx, name, capsys):
    x = R.E.to_float(C.quality_signals()[name])
    rows, bad = [], []
    for lay in C.QUALITY_LAYOUTS:
        ref = [gpu_ctx.encode_streams([x], FMT[lay], targetBitRate=rate)[0][0] for rate in S.RATES]
        e_ref = _errors(gpu_ctx, lay, x, ref)
        budgets = [len(s) for s in ref]
        got, info, infr = gpu_ctx.encode_rd_streams([x] * len(S.RATES), FMT[lay], budgets)
        e_got = _errors(gpu_ctx, lay, x, got)
        for k, rate in enumerate(S.RATES):
            rows.append("%-18s (%d,%d) %6d: B %5d E %12d | %5d %12d" % (name, lay[0], lay[1], rate, budgets[k], e_ref[k], len(got[k]), e_got[k]))
            if not (len(got[k]) <= budgets[k] and e_got[k] <= e_ref[k] and infr[k]["fits"]):
                bad.append(rows[-1])
        # the device's bytes are the restatement's (one budget per layout, the search being shared by all six)
        want = R.encode(C.quality_analysis(name), lay, budgets[2])
        assert got[2] == want[0] and C.info_of(infr[2]) == C.info_tuple(want[1])
    with capsys.disabled():
        print("\n" + "\n".join(rows))
    assert not bad, bad
