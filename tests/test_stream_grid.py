"""GPU (-m gpu): the readers of one window stream agree.  bf_enhance_device, bf_postfilter_device (with and without a lag) and
bf_resample_device read the same windows through csrc/stream_grid.h; what each carries or passes on is compared, bit for bit, with the
stream as tests/stft_np.py builds it, and every count with the model's integers."""
import numpy as np
import pytest

import stft_np
import util
from support import nat_restoring as nat

pytestmark = pytest.mark.gpu

M_TOTAL, N, N_FFT, HOP_S, MICS, LAG = 4, 24, 32, 8, (3, 1), 5


@pytest.mark.parametrize("hop", [10, 0], ids=["hop10", "whole_windows"])
def test_three_readers_of_one_stream_agree(nat, hop):
    """Two calls on fresh state, five windows and then one; hop = 10 reads behind the n - len offset, and its second call adds S = 10 < H,
    so every history shifts inside itself.  After each call every carried history is the last H samples of zeros(H) || stream, the
    identity resampler's output is the call's stream, and every count is the model's."""
    torch = util.torch_gpu()
    import enhance
    import postfilter
    util.configure_small(N)
    rng = np.random.default_rng([N, hop])
    en = enhance.Enhancer(rows=M_TOTAL, hop=hop or None, n_fft=N_FFT, hop_s=HOP_S)
    pfs = [postfilter.SpatialPostFilter(np.zeros((1, len(MICS))), MICS, 1, 1, hop or None, m_total=M_TOTAL, n_fft=N_FFT, hop_s=HOP_S, lag=lag) for lag in (0, LAG)]
    one = torch.ones(1, dtype=torch.float32, device="cuda")
    rs_state, rs_count = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    so_far, c = np.zeros((M_TOTAL, 0), np.float32), 0
    for F in (5, 1):
        w = rng.standard_normal((F, M_TOTAL, N)).astype(np.float32)
        assert (w != 0).all()
        x = stft_np.stream(w, N, hop)
        S = x.shape[1]
        assert S == F * (hop or N)
        so_far = np.concatenate([so_far, x], axis=1)
        count, c, _ = stft_np.advance(c, S, HOP_S)
        d_w = torch.from_numpy(w).cuda()
        d_out = torch.full((M_TOTAL, S), np.nan, dtype=torch.float32, device="cuda")
        _, en_count = en.push(d_w)
        pf_counts = [pf.gains(d_w, [0])[1] for pf in pfs]
        rc = nat.lib.bf_resample_device(d_w.data_ptr(), M_TOTAL, F, N, N, hop, None, one.data_ptr(), 1, 1, 1, rs_state.data_ptr(), 1.0, d_out.data_ptr(), S, None,
                                        None, rs_count.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0, nat.lib.bf_last_error()
        want = lambda rows, H: np.concatenate([np.zeros((len(rows), H), np.float32), so_far[list(rows)]], axis=1)[:, -H:]
        assert util.bits_differ(en.hist.cpu().numpy(), want(range(M_TOTAL), N_FFT - 1)) == ""
        for pf, lag in zip(pfs, (0, LAG)):
            assert util.bits_differ(pf.hist.cpu().numpy(), want(MICS, N_FFT - 1 + lag)) == "", lag
        assert util.bits_differ(d_out.cpu().numpy(), x) == ""
        assert en_count.cpu().tolist() == [count, 0] and en.last_count == count
        assert all(k.cpu().tolist() == [count, 0] for k in pf_counts) and all(pf.last_count == count for pf in pfs)
        assert rs_count.cpu().tolist() == [S, 0]
