"""The rule of the short pre-pass (dcsPrepassShort, csrc/dcs_package.h; no GPU needed): the 1994+ transform pairs point
i = l + 8 j of a frame's row (lane l = 0..7, j = 0..7, a point = two tile words) with point 128 - i, and in a batch whose rows
hold at most nb header bands the kernels of single-source batches leave the partner out for the first ZJ(nb) values of j.  That is
right exactly when the lowest partner of every such j lies behind the last word a frame of nb bands can fill."""
import dcsexplorer_amd as D


def last_word(nb):
    """bands of 7, 8, 13 x 16 and 32 samples from word 1 on (DecompressFrame's band lengths)"""
    return sum(([7, 8] + [16] * 13 + [32])[:nb])


def test_the_last_word_a_frame_can_fill():
    for nb in range(1, 17):
        assert D.api.prepass_short(nb)[1] == last_word(nb)
        if 2 <= nb <= 15:
            assert last_word(nb) == 15 + 16 * (nb - 2)
    assert D.api.prepass_short(0) == (8, 0) and D.api.prepass_short(40) == D.api.prepass_short(16)


def test_no_short_step_has_a_partner():
    """128 - (7 + 8 j) >= ceil((upTo + 1) / 2) for every j the function calls short, and -- so that nothing is given away -- not
    for the first j it does not"""
    for nb in range(1, 17):
        zj, up_to = D.api.prepass_short(nb)
        first_free = (up_to + 2) // 2               # ceil((up_to + 1) / 2)
        assert 0 <= zj <= 8
        for j in range(zj):
            assert 128 - (7 + 8 * j) >= first_free, (nb, j)
        if zj < 8:
            assert 128 - (7 + 8 * zj) < first_free, (nb, zj)


def test_the_table_of_the_band_counts():
    assert [D.api.prepass_short(nb)[0] for nb in range(9, 17)] == [8, 7, 6, 5, 4, 3, 2, 0]
    assert all(D.api.prepass_short(nb)[0] == 8 for nb in range(1, 10))
