"""GPU: the two-workgroup form of the descriptor head (csrc/sp_convs.hip: k_desc_head_sparse_2wg - patch quarters gathered by LDS-DMA through a
per-image buffer resource, two workgroups per CU) against k_desc_head_sparse<2>, the form it replaces, which the developer build keeps behind
SUPERSLAM_HIP_DESC_HEAD=1wg.  Same fp16 operands, same weight fragments in the same k order into the same fp32 accumulators: the descriptors are
equal BIT FOR BIT, compared as int16.  Both forms run through the test-only sship_sp_debug_desc_head on the same seeded maps and cells
(tests/_tail_ab.py): maps of 2 x 3, 8 x 12 and 47 x 172 cells, batches of 1, 2 and 5, 0 / 1 / 63 / 64 / 65 / 130 / max_kp keypoints per image with
max_kp = 200 (a ragged last workgroup), every batch of 2 or 5 with an image without keypoints, and keypoints on the four corners and all four edges
(every zero-padded tap; on the 2 x 3 map every cell is one) and in the interior.  A third run on the SHIPPED library takes the launcher's own
choice - the 32-keypoint latency form for these small grids, the two-workgroup form for the 5 x 1700-keypoint case - and must give the same bits."""
import numpy as np
import pytest

import _tail_ab as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def forms(weights_dir, tmp_path_factory):
    d = tmp_path_factory.mktemp("desc_head")
    return {name: T.run_worker("desc", env, weights_dir, str(d / (name + ".npz")))
            for name, env in (("1wg", {"SUPERSLAM_HIP_DESC_HEAD": "1wg"}), ("2wg", {"SUPERSLAM_HIP_DESC_HEAD": "2wg"}), ("shipped", {}))}


@pytest.mark.parametrize("hc,wc", T.MAPS)
@pytest.mark.parametrize("b", T.BATCHES)
def test_two_workgroup_head_is_bit_identical(forms, hc, wc, b):
    rows = 0
    for chc, cwc, cb, mk, counts, rot in T.desc_cases():
        if (chc, cwc, cb, mk) != (hc, wc, b, T.MAX_KP):
            continue
        key = T.desc_key(hc, wc, b, rot, mk)
        old, new, shipped = forms["1wg"][key], forms["2wg"][key], forms["shipped"][key]
        for i, n in enumerate(counts):
            assert (old[i, n:] == T.DESC_FILL).all() and (new[i, n:] == T.DESC_FILL).all(), (key, i, n)   # nothing written past the count
            assert n == 0 or old[i, :n].view(np.float16).astype(np.float32).any(), (key, i)                 # the oracle computed something
            rows += n
        bad = np.argwhere(old != new)
        assert bad.size == 0, (key, counts, len(bad), bad[:8].tolist())
        np.testing.assert_array_equal(old, shipped)
    print(f"{hc}x{wc} batch {b}: {rows} descriptor rows identical in the three forms")
    assert rows > 0


def test_launchers_own_choice_at_a_full_grid(forms):
    hc, wc, b, mk = T.BIG
    key = T.desc_key(hc, wc, b, 0, mk)
    old = forms["1wg"][key]
    assert old[0].view(np.float16).astype(np.float32).any() and (old[1] == T.DESC_FILL).all()
    for name in ("2wg", "shipped"):
        bad = np.argwhere(old != forms[name][key])
        assert bad.size == 0, (name, len(bad), bad[:8].tolist())
