"""GPU (-m gpu): the digest cache keyed by the plan's kernel family (DigestKey, csrc/beamformer_api.cpp).

lerp at N = 132 on a 16 x 16 grid (256 directions: 16 waves), frames of 32 rows.  With all 32 rows active a batch runs the lerp pair
sweep on rows of 16-byte cells (bf_last_das_rows() == 2), with 16 of them on rows of sample pairs (1): two families whose plans show
the same mic_chunk, row_stride and lead, and whose digests address different row layouts.  Calls that alternate between the two, at
two and at three frames, each report their own family and give the oracle's maps bit for bit.

A table without structure hands the 16-microphone launch to the direction-outer family (3) while its digest is built; the slot keeps
the key of the sweep plan the caller arrives with, so the same call again finds the slot and replans: family 3 both times, equal bits."""
import numpy as np
import pytest

import batched_cases as BC
import util
from support import nat
from util import ALGOS

pytestmark = pytest.mark.gpu

N, GRID, M_TOTAL, T, PMAX = 132, (16, 16), 32, 8, 30.0


def _case(name, n, kind, family):
    if name not in BC.EXTRA:
        BC.EXTRA[name] = BC.Case(name, family, ("lerp",), M_TOTAL, n, N, GRID[0], GRID[1], T, PMAX, kind, "sorted", 3)
    return BC.EXTRA[name]


def _load(nat, name):
    t = np.ascontiguousarray(BC.table(name, "lerp")).ravel()
    nat.lib.load_coefficients_lerp(nat.fptr(t), t.size)
    nat.check()


def _das(nat, name, frames):
    """bf_das_device on the first `frames` frames of the case over the full grid -> (maps float32 [frames, D], variant, rows)."""
    torch = util.torch_gpu()
    c, d = BC.case_of(name), BC.data(name)
    D = c.X * c.Y
    d_sig = torch.from_numpy(d.frames[:frames].copy()).cuda()
    mics = d.mics.copy()
    out = torch.full((frames, D), float("nan"), dtype=torch.float32, device="cuda")
    assert nat.lib.bf_das_device(ALGOS["lerp"], d_sig.data_ptr(), c.M_total, out.data_ptr(), D, frames, nat.iptr(mics), mics.size, 0, D,
                                 torch.cuda.current_stream().cuda_stream) == 0, nat.check()
    torch.cuda.synchronize()
    return out.cpu().numpy(), nat.lib.bf_last_das_variant(), nat.lib.bf_last_das_rows()


def _configure(c):
    from interface import config
    config.configure(N_MICROPHONES=c.M_total, N_SAMPLES=c.N, MAX_RES_X=c.X, MAX_RES_Y=c.Y, N_TAPS=c.T)


def test_alternating_row_layouts_keep_their_families(nat, oracle_lib):
    cells, pairs = _case("family_key_32of32", 32, "smooth", 8), _case("family_key_16of32", 16, "smooth", 8)
    want = {c.name: BC.want(oracle_lib, c.name, "lerp") for c in (cells, pairs)}
    try:
        _configure(cells)
        for c, frames, rows in ((cells, 2, 2), (pairs, 2, 1), (cells, 3, 2), (pairs, 2, 1)):
            _load(nat, c.name)                                  # (a table has one column per active microphone)
            got, variant, layout = _das(nat, c.name, frames)
            print("%s, %d frames: family %d rows %d" % (c.name, frames, variant, layout))
            assert (variant, layout) == (8, rows), (c.name, frames)
            for f in range(frames):
                why = util.bits_differ(got[f], want[c.name][f])
                assert not why, "%s, frame %d of %d: %s" % (c.name, f, frames, why)
    finally:
        util.configure("cfg1")


def test_direction_outer_slot_is_found_again(nat, oracle_lib):
    c = _case("family_key_random_16of32", 16, "random", 3)
    want = BC.want(oracle_lib, c.name, "lerp")
    try:
        _configure(c)
        _load(nat, c.name)
        first, variant, layout = _das(nat, c.name, 2)           # builds the grouped digest, counts its re-reads, replans direction-outer
        assert (variant, layout) == (3, 0)
        again, variant, layout = _das(nat, c.name, 2)           # the sweep plan's key finds the slot: replanned from the cache
        assert (variant, layout) == (3, 0)
        for f in range(2):
            why = util.bits_differ(first[f], want[f])
            assert not why, "frame %d: %s" % (f, why)
        assert again.tobytes() == first.tobytes()
    finally:
        util.configure("cfg1")
