"""GPU: convPb's whole-tile stores (csrc/sp_convs.hip: k_convpb_stream<true> - the 16 x 68 logits of a tile through a wave-private LDS patch,
then lane-linear 16-byte stores) against the store path they replace (one 64-byte piece per pixel and M-tile), which the developer build keeps
behind SUPERSLAM_HIP_CONVPB=pieces.  Prefetch and MFMA order are the same, so channels 0..64 are equal BIT FOR BIT, compared as uint32, at
P = 1, 15, 16, 17, 33 pixels, at 80 (five tiles on two workgroups: three waves have no tile) and at 197 (a ragged 13th tile); floats 65..67 of every
row are zero in the new form (the old one never writes them); the rows behind the last pixel are not touched; and keypoints, scores and descriptors
of sship_sp_extract_batch_device on two 64 x 96 frames are the same.  The shipped library's single path is the third run."""
import numpy as np
import pytest

import _tail_ab as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def forms(weights_dir, tmp_path_factory):
    d = tmp_path_factory.mktemp("convpb")
    return {name: T.run_worker("convpb", env, weights_dir, str(d / (name + ".npz")))
            for name, env in (("pieces", {"SUPERSLAM_HIP_CONVPB": "pieces"}), ("whole", {"SUPERSLAM_HIP_CONVPB": "whole"}), ("shipped", {}))}


@pytest.mark.parametrize("p", T.CONVPB_P)
def test_logits_are_bit_identical_and_padding_is_zero(forms, p):
    old = forms["pieces"]["l_%d" % p]
    assert old.shape == (p + 2, 68) and (old[:p, 65:] == T.LOGIT_FILL).all()   # the oracle leaves the padding alone
    assert (old[:p, :65] != T.LOGIT_FILL).all() and np.isfinite(old[:p, :65].view(np.float32)).all()
    for name in ("whole", "shipped"):
        new = forms[name]["l_%d" % p]
        np.testing.assert_array_equal(new[:p, :65], old[:p, :65])
        assert (new[:p, 65:] == 0).all(), name
        assert (new[p:] == T.LOGIT_FILL).all() and (old[p:] == T.LOGIT_FILL).all(), name   # ragged last tile: only the valid rows


def test_extraction_is_unchanged_on_a_64x96_frame(forms):
    old = forms["pieces"]
    assert old["n"].min() > 0
    for name in ("whole", "shipped"):
        new = forms[name]
        np.testing.assert_array_equal(new["n"], old["n"])
        for i, n in enumerate(old["n"]):
            np.testing.assert_array_equal(new["kp"][i, :n], old["kp"][i, :n])       # x, y and score, as uint32
            np.testing.assert_array_equal(new["desc"][i, :n], old["desc"][i, :n])
    print("64x96 frames:", old["n"].tolist(), "keypoints, identical")
