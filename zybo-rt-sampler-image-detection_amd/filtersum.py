"""Filter-and-sum beams on the device path: null steering, and any fixed beamformer a caller brings along as taps.

Every other audio beam here is delay-and-sum, so a beam aimed at one talker still carries the other at sidelobe level -- and on a
14 cm aperture "sidelobe level" is a few dB.  Any fixed beamformer is a filter-and-sum: one FIR per (beam, microphone), then a sum
over the microphones (bf_filter_sum_device, include/beamformer_hip.h has the definition).  `design_lcmv` designs such filters on the
host in float64: unit response in the look direction, zero response in up to a few null directions, at every frequency bin of the
band (LCMV: linearly constrained minimum variance, for spatially white noise).  `FilterSumListener` runs them.

Recipe, two talkers:
    bl = BeamListener("lerp");  maps = bl.maps(d_frames);  offs, _, _ = bl.sources(maps, 2, radius)
    tau = lib.directions.calculate_delays().reshape(-1, bl.n)
    fs_ = FilterSumListener.cross_null(tau, offs[0].cpu().numpy(), bl.offset_per_dir, hop=hop)    # beam i: source i heard, the others nulled
    out = fs_.listen(d_frames);  fs_.advance(d_frames);  audio = fs_.audio(out)                    # delayed by fs_.delay samples

Beams that follow a tracker without a host round trip: `cross_null` needs the offsets on the host and designs there.  A listener
built by `for_slots` keeps one beam per tracker slot and re-designs on the device (bf_lcmv_design_device: the same design, float64,
written into the taps the beams read), so tracker -> designer -> beams is one stream of launches and captures into one graph:
    fs_ = FilterSumListener.for_slots(tau, slots, bl.offset_per_dir, hop=hop)
    offsets, ids, pos = tracker.update(offs)
    status, kept = fs_.retarget(offsets[-1]);  out = fs_.listen(d_frames)                           # beam s: slot s heard, the other sources nulled
`design_slots` is the host statement of that call: the fallback without a device, and what the tests hold the device to.

Interference no slot names (a talker under another's main-lobe skirt, a reflection, a fan): `adapt` designs the same listener's taps
from the covariance of the frames themselves (bf_mvdr_design_device: MVDR, unit response towards each slot, minimum output power):
    status, fallback = fs_.adapt(d_frames, offsets[-1]);  out = fs_.listen(d_frames)
`design_mvdr` / `design_mvdr_slots` are its host statements.  Limit: frames in which the look talker is as loud as the interference
make sample-covariance MVDR cancel part of the look signal as well (self-cancellation); adapt on frames where it is weak.
The cure is `learn`: the covariance is state on the device that carries from call to call (bf_mvdr_learn_device), every frame has a
weight read on the device -- 0 where the look talker speaks -- and `forget` sets how long old frames count; `reaim` designs new taps
from the state as it stands when the tracker moves a slot, `forget_all` empties it:
    offsets, ids, pos, match, counts = tracker.update(offs)
    status, fallback, used = fs_.learn(d_frames, offsets[-1], weights=(match[:, s] < 0).double(), forget=0.9)
    status, fallback = fs_.reaim(offsets[-1]);  out = fs_.listen(d_frames)
`mvdr_learn` / `design_mvdr_learned` are its host statements.
A caller with weights of their own passes `taps=` to FilterSumListener."""
import numpy as np

from carried import CarriedBeams
from interface import config
from lib import _native as nat
from lib._native import _torch, call

MAX_BEAMS = 16
MAX_SLOTS = 8           # BF_LCMV_MAX_SOURCES
MAX_DESIGN_TAPS = 1024  # BF_LCMV_MAX_TAPS


def band_bins(n_taps, band, fs=None):
    """The bins k of the n_taps-point frequency grid, 0 <= k <= n_taps // 2, with k * fs / n_taps inside band = (f_lo, f_hi), inclusive."""
    fs = float(config.SAMPLE_RATE if fs is None else fs)
    T = int(n_taps)
    k = np.arange(T // 2 + 1)
    f = k * fs / T
    return k[(f >= float(band[0])) & (f <= float(band[1]))]


def _design_args(tau, n_taps, band, fs, rho=None):
    """What every designer checks of its design: tau [D, M], n_taps >= 1, rho in (0, 1] where the design has one, a band that holds a
    bin -> (tau float64, T = n_taps, the in-band bins)."""
    tau = np.asarray(tau, dtype=np.float64)
    if tau.ndim != 2:
        raise ValueError("tau must be [D, M], got shape %s" % (tau.shape,))
    T = int(n_taps)
    if T < 1:
        raise ValueError("n_taps must be >= 1, got %d" % T)
    if rho is not None and not 0.0 < float(rho) <= 1.0:
        raise ValueError("rho must be in (0, 1], got %g" % rho)
    fs = float(config.SAMPLE_RATE if fs is None else fs)
    bins = band_bins(T, band, fs)
    if bins.size == 0:
        raise ValueError("no bin of the %d-point grid lies in the band (%g, %g) at fs = %g" % (T, band[0], band[1], fs))
    return tau, T, bins


def design_lcmv(tau, look, nulls=None, n_taps=65, band=(3000.0, 8000.0), rho=0.95, fs=None):
    """Null-steering filter-and-sum taps by frequency sampling, designed in float64.

    tau   float64 [D, M]: delays in samples per (direction, active microphone) -- lib.directions.calculate_delays() reshaped.
          Microphone m LEADS by tau[d][m] (synth.s3_plane_wave), so the response of one beam's taps g [M, T] to a plane wave from
          d at w rad/sample is  H(w, d) = sum_m (sum_t g[m][t] e^{-jwt}) e^{+jw tau[d][m]}   (`response`).
    look  B flat direction indices, one beam each.
    nulls per beam a list of up to J direction indices (None: no nulls anywhere).
    ->    (taps float32 [B, M, T], kept bool [B, K, J]);  K = len(band_bins(n_taps, band, fs)), the in-band bins in ascending order.

    For every in-band bin k: w = 2 pi k / T, c_d[m] = e^{+jw tau[d][m]}, C = [c_look, kept nulls], target f = (e^{-jw(T-1)/2}, 0, ..),
    u = C (C^H C)^{-1} conj(f), gains G_k[m] = conj(u[m]): the minimum-norm gains with H(w, look) = e^{-jw(T-1)/2} and H(w, null) = 0.
    Bins outside the band are zero; the taps are the inverse real DFT of the G_k (which keeps the real part of a DC or Nyquist gain),
    rounded once to float32.  At a bin a null is DROPPED if |c^H c'| / M > rho against the look vector or a null already kept at
    that bin (tried in the order given): it cannot be told from them there, and forcing it would blow the white-noise gain up.
    `kept` reports the outcome; entries past a beam's own list are False.

    A beam's output is the look direction's signal delayed by (T - 1) / 2 samples and band-limited.  With no nulls the design is
    band-limited delay-and-sum with exact fractional delays."""
    tau, T, bins = _design_args(tau, n_taps, band, fs, rho)
    D, M = tau.shape
    look = [int(d) for d in np.asarray(look).ravel()]
    B = len(look)
    if B < 1:
        raise ValueError("look is empty")
    nulls = [[] for _ in look] if nulls is None else [[int(d) for d in np.asarray(row).ravel()] for row in nulls]
    if len(nulls) != B:
        raise ValueError("nulls must list the nulls of every beam: %d beams, %d lists" % (B, len(nulls)))
    for d in look + [d for row in nulls for d in row]:
        if d < 0 or d >= D:
            raise ValueError("direction %d is outside tau's %d directions" % (d, D))
    J = max([len(row) for row in nulls] + [0])
    kept = np.zeros((B, bins.size, J), dtype=bool)
    G = np.zeros((B, M, T // 2 + 1), dtype=np.complex128)
    for b in range(B):
        for i, k in enumerate(bins):
            w = 2.0 * np.pi * k / T
            cols = [np.exp(1j * w * tau[look[b]])]
            for j, d in enumerate(nulls[b]):
                c = np.exp(1j * w * tau[d])
                if all(abs(np.vdot(c, other)) / M <= rho for other in cols):
                    cols.append(c)
                    kept[b, i, j] = True
            C = np.stack(cols, axis=1)                                      # [M, 1 + kept nulls]
            f = np.zeros(C.shape[1], dtype=np.complex128)
            f[0] = np.exp(-1j * w * (T - 1) / 2.0)
            u = C @ np.linalg.solve(C.conj().T @ C, f.conj())
            G[b, :, k] = u.conj()
    taps = np.fft.irfft(G, n=T, axis=2)
    return np.ascontiguousarray(taps, dtype=np.float32), kept


def slot_directions(offsets, offset_per_dir, n_dirs):
    """The direction of every slot of a row of offsets, -1 where the slot is no source: an entry is a source iff it is >= 0, a
    multiple of offset_per_dir and names one of the n_dirs directions (the tracker's rule)."""
    step = int(offset_per_dir)
    if step < 1:
        raise ValueError("offset_per_dir must be >= 1, got %d" % step)
    return [int(o) // step if int(o) >= 0 and int(o) % step == 0 and int(o) // step < int(n_dirs) else -1 for o in np.asarray(offsets).ravel()]


def design_slots(tau, offsets, offset_per_dir, n_taps=65, band=(3000.0, 8000.0), rho=0.95, fs=None):
    """One beam per SLOT of a row of offsets (what BeamListener.sources / SourceTracker wrote), designed on the host in float64: the
    statement of bf_lcmv_design_device (include/beamformer_hip.h), on top of design_lcmv.

    Beam i belongs to slot i -- slots are not compacted as cross_null compacts them, a tracker slot keeps its beam.  Its look
    direction is slot i's, its nulls are every other slot that is a source, tried in slot order.  A slot that is no source
    (`slot_directions`) gets all-zero taps, status 1 and no kept entry; a designed slot gets status 0.
    ->    (taps float32 [S, M, T], kept int32 [S, K, S], status int32 [S]);  kept[i][k][j] = 1 iff slot j is a kept null of beam i at
          in-band bin k (the diagonal, slots that are no source and dropped nulls are 0)."""
    tau, T, bins = _design_args(tau, n_taps, band, fs, rho)
    dirs = slot_directions(offsets, offset_per_dir, tau.shape[0])
    S, K = len(dirs), bins.size
    if S < 1:
        raise ValueError("offsets is empty")
    if S > tau.shape[1]:
        raise ValueError("%d slots but %d microphones: more constraints than microphones make the system singular" % (S, tau.shape[1]))
    taps = np.zeros((S, tau.shape[1], T), dtype=np.float32)
    kept = np.zeros((S, K, S), dtype=np.int32)
    status = np.array([0 if d >= 0 else 1 for d in dirs], dtype=np.int32)
    live = [i for i in range(S) if dirs[i] >= 0]
    if live:
        others = [[j for j in live if j != i] for i in live]
        g, k = design_lcmv(tau, [dirs[i] for i in live], [[dirs[j] for j in row] for row in others], n_taps=T, band=band, rho=rho, fs=fs)
        for b, i in enumerate(live):
            taps[i] = g[b]
            for col, j in enumerate(others[b]):
                kept[i, :, j] = k[b, :, col]
    return taps, kept, status


def _mvdr_snapshots(frames, mics, T, bins, seg_first, seg_hop, segs, window, min_frames=1):
    """The snapshots of bf_mvdr_design_device in float64 -> (snap complex128 [F * segs, K, M], segs as chosen)."""
    x = np.asarray(frames)
    if x.ndim != 3 or x.dtype != np.float32:
        raise ValueError("frames must be float32 [F, M_total, N], got %s %s" % (x.dtype, x.shape))
    mics = np.asarray(mics).astype(np.int64).ravel()
    F, m_total, N = x.shape
    M = int(mics.size)
    if M < 1 or mics.min() < 0 or mics.max() >= m_total:
        raise ValueError("mics names a row outside the frames' %d rows" % m_total)
    if T > N:
        raise ValueError("n_taps must be in [1, N = %d], got %d" % (N, T))
    seg_first, seg_hop = int(seg_first), int(seg_hop)
    if seg_first < 0 or seg_hop < 1:
        raise ValueError("seg_first must be >= 0 and seg_hop >= 1, got %d and %d" % (seg_first, seg_hop))
    segs = (N - seg_first - T) // seg_hop + 1 if segs is None else int(segs)
    if F < min_frames or segs < 1 or seg_first + (segs - 1) * seg_hop + T > N:
        raise ValueError("segments [%d + q * %d, + %d), q < %d, do not fit windows of %d samples" % (seg_first, seg_hop, T, segs, N))
    win = np.ones(T) if window is None else np.asarray(window, dtype=np.float64)
    if win.shape != (T,):
        raise ValueError("window must be [n_taps = %d], got shape %s" % (T, win.shape))
    r = np.arange(T)
    table = np.cos(2.0 * np.pi * r / T) - 1j * np.sin(2.0 * np.pi * r / T)            # e^{-j 2 pi r / T}
    E = table[(np.arange(T)[:, None] * bins[None, :]) % T]                           # [T, K]: the integer (k t) mod T picks the entry
    snap = np.empty((F * segs, bins.size, M), dtype=np.complex128)
    with np.errstate(all="ignore"):                                                  # NaN and Inf samples are an input like any other
        for f in range(F):
            for q in range(segs):
                s0 = seg_first + q * seg_hop
                seg = x[f][mics, s0:s0 + T].astype(np.float64) * win[None, :]
                snap[f * segs + q] = (seg @ E).T
    return snap, segs


def _mvdr_gains_of(cov, tau, dirs, bins, T, loading):
    """Loading, factor and solve of bf_mvdr_design_device on a covariance complex128 [K, M, M], for the directions `dirs` (-1: no
    source, zero gains) -> (gains complex128 [B, K, M], fallback int32 [K])."""
    loading = float(loading)
    if not (np.isfinite(loading) and loading > 0.0):
        raise ValueError("loading must be finite and > 0, got %g" % loading)
    for d in dirs:
        if d >= tau.shape[0]:
            raise ValueError("direction %d is outside tau's %d directions" % (d, tau.shape[0]))
    K, M = bins.size, tau.shape[1]
    with np.errstate(all="ignore"):
        fallback = np.zeros(K, dtype=np.int32)
        G = np.zeros((len(dirs), K, M), dtype=np.complex128)
        for i, k in enumerate(bins):
            tr = float(np.sum(cov[i].diagonal().real))
            if np.isfinite(tr) and tr > 0.0:
                loaded = cov[i] + (loading * tr / M) * np.eye(M)
            else:
                loaded = np.eye(M, dtype=np.complex128)
                fallback[i] = 1
            L = np.linalg.cholesky(loaded)
            w = 2.0 * np.pi * k / T
            for b, d in enumerate(dirs):
                if d < 0:
                    continue
                c = np.exp(1j * w * tau[d])
                y = np.linalg.solve(L, c)
                z = np.linalg.solve(L.conj().T, y)
                u = z * np.exp(1j * w * (T - 1) / 2.0) / np.sum(np.abs(y) ** 2)
                G[b, i] = u.conj()
    return G, fallback


def _mvdr_gains(frames, mics, tau, dirs, n_taps, band, loading, seg_first, seg_hop, segs, window, fs):
    """The float64 statement of bf_mvdr_design_device up to the gains, for the directions `dirs` (-1: no source, zero gains).
    -> (gains complex128 [B, K, M], fallback int32 [K], bins)."""
    tau, T, bins = _design_args(tau, n_taps, band, fs)
    if np.asarray(mics).size != tau.shape[1]:
        raise ValueError("mics lists %d rows, tau is for %d microphones" % (np.asarray(mics).size, tau.shape[1]))
    snap, _ = _mvdr_snapshots(frames, mics, T, bins, seg_first, seg_hop, segs, window)
    with np.errstate(all="ignore"):
        cov = np.einsum("pka,pkb->kab", snap, snap.conj()) / snap.shape[0]
    G, fallback = _mvdr_gains_of(cov, tau, dirs, bins, T, loading)
    return G, fallback, bins


def _taps_of_gains(G, bins, T):
    """design_lcmv's last two lines: gains [B, K, M] on the whole grid, irfft, one rounding to float32 -> [B, M, T]."""
    B, K, M = G.shape
    full = np.zeros((B, M, T // 2 + 1), dtype=np.complex128)
    full[:, :, bins] = G.transpose(0, 2, 1)
    return np.ascontiguousarray(np.fft.irfft(full, n=T, axis=2), dtype=np.float32)


def design_mvdr(frames, mics, tau, look, n_taps=65, band=(3000.0, 8000.0), loading=0.1, seg_first=0, seg_hop=16, segs=None, window=None, fs=None):
    """Adaptive (MVDR) filter-and-sum taps from the covariance of the frames themselves, in float64: the host statement of
    bf_mvdr_design_device (include/beamformer_hip.h has the definition) for the look directions `look`, one beam each.

    frames float32 [F, M_total, N]; mics the M rows of a frame the beams use (tau's microphones, in its order); tau as design_lcmv.
    Snapshots: the T = n_taps point DFT, at the in-band bins, of `window` (float64 [T], None: rectangular) times the T samples from
    seg_first + q * seg_hop of every window, q < segs (None: as many as fit).  Per bin: R = mean of X X^H over the snapshots,
    R' = R + (loading tr R / M) I, gains u = R'^{-1} c conj(f0) / (c^H R'^{-1} c) with c = e^{+jw tau[look]}, f0 = e^{-jw(T-1)/2}: unit
    response towards `look`, minimum output power for THESE frames -- whatever interferes in them is suppressed without being named.
    A bin whose trace is not finite and > 0 (silence, NaN, Inf) uses R' = I, design_lcmv's beam without nulls, and reports fallback 1.
    ->    (taps float32 [B, M, T], fallback int32 [K]).

    Limit: if the look talker is in the frames about as loud as the interference, any mismatch between c and its true wavefront
    (the T-sample snapshot is a narrowband model; delays reach 15 samples) makes the design cancel part of it too."""
    look = [int(d) for d in np.asarray(look).ravel()]
    if not look:
        raise ValueError("look is empty")
    if min(look) < 0:
        raise ValueError("direction %d is outside tau's directions" % min(look))
    G, fallback, bins = _mvdr_gains(frames, mics, tau, look, n_taps, band, loading, seg_first, seg_hop, segs, window, fs)
    return _taps_of_gains(G, bins, int(n_taps)), fallback


def design_mvdr_slots(frames, mics, tau, offsets, offset_per_dir, n_taps=65, band=(3000.0, 8000.0), loading=0.1, seg_first=0, seg_hop=16, segs=None,
                      window=None, fs=None):
    """design_mvdr with design_slots' slot semantics: beam i looks at slot i of a row of offsets; a slot that is no source
    (`slot_directions`) gets all-zero taps and status 1.  The other slots are not nulls of a beam -- only the data decides.
    ->    (taps float32 [S, M, T], fallback int32 [K], status int32 [S])."""
    tau, T, _ = _design_args(tau, n_taps, band, fs)
    dirs = slot_directions(offsets, offset_per_dir, tau.shape[0])
    if not dirs:
        raise ValueError("offsets is empty")
    G, fallback, bins = _mvdr_gains(frames, mics, tau, dirs, T, band, loading, seg_first, seg_hop, segs, window, fs)
    return _taps_of_gains(G, bins, T), fallback, np.array([0 if d >= 0 else 1 for d in dirs], dtype=np.int32)


def mvdr_learn(acc, mass, frames, mics, weights=None, forget=1.0, n_taps=65, band=(3000.0, 8000.0), seg_first=0, seg_hop=16, segs=None, window=None, fs=None):
    """The state of bf_mvdr_learn_device advanced by one call, in float64 on the host: its chains one for one.

    acc complex128 [K, M, M], the weighted sum of X X^H per in-band bin, and mass, the weights' sum times segs; zeros are the empty
    state (acc None: empty).  frames float32 [F, M_total, N] (F = 0: nothing happens), mics, the segments and the window as
    design_mvdr.  weights [F] or None (all 1): frame f is learned iff its weight is finite and > 0; +-0 is skipped silently, a NaN, an
    Inf or a negative weight is skipped and counted.  Per learned frame, in ascending f:
        acc = forget * acc;  acc = acc + w_f * X_p X_p^H for every segment q in ascending order;  mass = forget * mass + w_f * segs
    with forget in (0, 1].  A skipped frame changes nothing: forgetting counts learned frames, not time.
    ->    (acc complex128 [K, M, M] (a new array, exactly Hermitian), mass float, used int32 [2] = (learned, refused))."""
    T = int(n_taps)
    if T < 1:
        raise ValueError("n_taps must be >= 1, got %d" % T)
    bins = band_bins(T, band, fs)
    if bins.size == 0:
        raise ValueError("no bin of the %d-point grid lies in the band (%g, %g)" % (T, band[0], band[1]))
    forget = float(forget)
    if not 0.0 < forget <= 1.0:
        raise ValueError("forget must be in (0, 1], got %g" % forget)
    snap, segs = _mvdr_snapshots(frames, mics, T, bins, seg_first, seg_hop, segs, window, min_frames=0)
    F, K, M = snap.shape[0] // segs, bins.size, snap.shape[2]
    acc = np.zeros((K, M, M), dtype=np.complex128) if acc is None else np.asarray(acc, dtype=np.complex128)
    if acc.shape != (K, M, M):
        raise ValueError("acc must be [K = %d, M = %d, M], got shape %s" % (K, M, acc.shape))
    w_all = np.ones(F) if weights is None else np.asarray(weights, dtype=np.float64).ravel()
    if w_all.shape != (F,):
        raise ValueError("weights must be [F = %d], got shape %s" % (F, w_all.shape))
    re, im, mass = acc.real.copy(), acc.imag.copy(), float(mass)
    learned = refused = 0
    with np.errstate(all="ignore"):
        for f in range(F):
            w = float(w_all[f])
            if not (np.isfinite(w) and w > 0.0):
                refused += 0 if w == 0.0 else 1
                continue
            learned += 1
            re, im = forget * re, forget * im
            for q in range(segs):
                xr, xi = snap[f * segs + q].real, snap[f * segs + q].imag                        # [K, M]
                re = re + w * (xr[:, :, None] * xr[:, None, :] + xi[:, :, None] * xi[:, None, :])     # X[a] conj(X[b])
                im = im + w * (xi[:, :, None] * xr[:, None, :] - xr[:, :, None] * xi[:, None, :])
            mass = forget * mass + w * float(segs)
    out = np.empty((K, M, M), dtype=np.complex128)
    out.real, out.imag = re, im
    return out, mass, np.array([learned, refused], dtype=np.int32)


def design_mvdr_learned(acc, mass, tau, offsets, offset_per_dir, n_taps=65, band=(3000.0, 8000.0), loading=0.1, fs=None):
    """design_mvdr_slots' taps from a learned state (`mvdr_learn`) instead of frames: the covariance is acc / mass, all zeros where the
    mass is not > 0 -- every bin then falls back to the beam without nulls.  Loading, factor, solve and taps are design_mvdr's.
    ->    (taps float32 [S, M, T], fallback int32 [K], status int32 [S])."""
    tau, T, bins = _design_args(tau, n_taps, band, fs)
    dirs = slot_directions(offsets, offset_per_dir, tau.shape[0])
    if not dirs:
        raise ValueError("offsets is empty")
    acc = np.asarray(acc, dtype=np.complex128)
    if acc.shape != (bins.size, tau.shape[1], tau.shape[1]):
        raise ValueError("acc must be [K = %d, M = %d, M], got shape %s" % (bins.size, tau.shape[1], acc.shape))
    mass = float(mass)
    cov = np.zeros_like(acc)
    if mass > 0.0:
        with np.errstate(all="ignore"):
            cov.real, cov.imag = acc.real / mass, acc.imag / mass
    G, fallback = _mvdr_gains_of(cov, tau, dirs, bins, T, loading)
    return _taps_of_gains(G, bins, T), fallback, np.array([0 if d >= 0 else 1 for d in dirs], dtype=np.int32)


def response(taps, tau_row, w):
    """H(w, d) of one beam in float64: taps [M, T], tau_row float64 [M] = tau[d], w rad/sample (a scalar or an array) -> complex, w's shape."""
    g = np.asarray(taps, dtype=np.float64)
    tau_row = np.asarray(tau_row, dtype=np.float64)
    if g.ndim != 2 or tau_row.shape != (g.shape[0],):
        raise ValueError("taps must be [M, T] and tau_row [M], got %s and %s" % (g.shape, tau_row.shape))
    w = np.asarray(w, dtype=np.float64)
    t = np.arange(g.shape[1], dtype=np.float64)
    flat = w.reshape(-1)
    per_mic = np.exp(-1j * flat[:, None] * t[None, :]) @ g.T                # [W, M]: sum_t g[m][t] e^{-jwt}
    h = np.sum(per_mic * np.exp(1j * flat[:, None] * tau_row[None, :]), axis=1)
    return h.reshape(w.shape) if w.ndim else complex(h[0])


class FilterSumListener(CarriedBeams):
    """B filter-and-sum beams over the microphone rows `mics` (default: lib.directions.active_microphones(), as BeamListener).
    `taps`: float32 [B, M, T], g[b][m][t] for microphone row mics[m] -- from `design_lcmv`, `cross_null`, or a caller's own design.
    `hop`: samples between the starts of consecutive frames, as given to the ingest (None: independent windows, every window starts
    from silence).  With a hop the carried state is one frame, the last one of the batch before: `advance` sets it, `reset` clears
    it, `listen` only reads it.  `.delay` is (T - 1) / 2, the delay of a design_lcmv beam in samples."""

    def __init__(self, taps, mics=None, hop=None, device="cuda"):
        g = np.ascontiguousarray(taps, dtype=np.float32)
        if g.ndim == 2:
            g = g[None]
        if g.ndim != 3 or g.shape[2] < 1:
            raise ValueError("taps must be [B, M, T], got shape %s" % (g.shape,))
        if mics is None:
            from lib.directions import active_microphones
            mics, _ = active_microphones()
        self.mics = np.ascontiguousarray(np.asarray(mics).astype(np.int32).ravel())
        self.n = int(self.mics.size)
        B, M, T = g.shape
        N = config.N_SAMPLES
        if B < 1 or B > MAX_BEAMS:
            raise ValueError("1 .. %d beams, got %d" % (MAX_BEAMS, B))
        if M != self.n:
            raise ValueError("taps are for %d microphones, mics lists %d" % (M, self.n))
        if T > N:
            raise ValueError("n_taps = %d > N_SAMPLES = %d" % (T, N))
        hop = 0 if hop is None else int(hop)
        if hop < 0 or hop > N:
            raise ValueError("hop must be in [0, N_SAMPLES = %d] (0 or None: independent windows), got %d" % (N, hop))
        if hop > 0 and T - 1 > hop:
            raise ValueError("n_taps - 1 = %d samples of history do not fit hop = %d" % (T - 1, hop))
        self.taps, self.B, self.T, self.hop, self.device = g, B, T, hop, device
        self.delay = (T - 1) / 2.0
        self.d_taps = _torch().from_numpy(g).to(device)
        self.dirs = self.kept = None                    # set by cross_null
        self.d_tau = None                               # set by for_slots: the device-side designer's state
        self.d_snap = self.d_cov = self.d_chol = self.d_fallback = self._window = self._mvdr_key = None      # adapt's and learn's workspaces
        self.d_acc = self.d_mass = self.d_used = None   # learn's state: the carried covariance

    @classmethod
    def cross_null(cls, tau, offsets, offset_per_dir, mics=None, hop=None, device="cuda", **design):
        """One beam per valid source offset, every other valid source its null.  `offsets`: a HOST row of what BeamListener.sources /
        SourceTracker wrote; an entry is a source iff it is >= 0, a multiple of offset_per_dir and names one of tau's directions
        (the tracker's rule).  **design goes to design_lcmv (n_taps, band, rho, fs).  The listener's `.dirs` lists the beams'
        directions in the order of the valid offsets, `.kept` is design_lcmv's."""
        tau = np.asarray(tau, dtype=np.float64)
        dirs = [d for d in slot_directions(offsets, offset_per_dir, tau.shape[0]) if d >= 0]
        if not dirs:
            raise ValueError("offsets holds no valid source")
        nulls = [[d for j, d in enumerate(dirs) if j != i] for i in range(len(dirs))]
        taps, kept = design_lcmv(tau, dirs, nulls, **design)
        self = cls(taps, mics=mics, hop=hop, device=device)
        self.dirs, self.kept = dirs, kept
        return self

    @classmethod
    def for_slots(cls, tau, slots, offset_per_dir, hop=None, n_taps=65, band=(3000.0, 8000.0), rho=0.95, fs=None, mics=None, device="cuda"):
        """A listener with B = `slots` beams whose taps are designed ON THE DEVICE: beam s belongs to slot s of the offsets given to
        `retarget` (design_slots' semantics).  The taps start at zero (silent beams); tau is uploaded once, the designer's outputs
        (d_gains float64 [slots, K, M, 2], d_kept int32 [slots, K, slots], d_status int32 [slots]) are allocated once.  `.taps`, the
        host copy, is None until `taps_host()` fetches it."""
        torch = _torch()
        tau, T, bins = _design_args(tau, n_taps, band, fs, rho)
        S, step = int(slots), int(offset_per_dir)
        if S < 1 or S > MAX_SLOTS:
            raise ValueError("1 .. %d slots, got %d" % (MAX_SLOTS, S))
        if S > tau.shape[1]:
            raise ValueError("%d slots but %d microphones: more constraints than microphones" % (S, tau.shape[1]))
        if T > MAX_DESIGN_TAPS:
            raise ValueError("1 .. %d taps, got %d" % (MAX_DESIGN_TAPS, T))
        if step < 1:
            raise ValueError("offset_per_dir must be >= 1, got %d" % step)
        self = cls(np.zeros((S, tau.shape[1], T), dtype=np.float32), mics=mics, hop=hop, device=device)
        self.taps = None
        self.bins, self.rho, self.offset_per_dir, self.n_dirs = bins, float(rho), step, int(tau.shape[0])
        self.d_tau = torch.from_numpy(np.ascontiguousarray(tau)).to(device)
        self.d_gains = torch.zeros((S, bins.size, self.n, 2), dtype=torch.float64, device=device)
        self.d_kept = torch.zeros((S, bins.size, S), dtype=torch.int32, device=device)
        self.d_status = torch.ones((S,), dtype=torch.int32, device=device)
        return self

    def _check_slots(self, who, d_offsets):
        """What retarget and adapt ask of the listener and of d_offsets -> torch."""
        torch = _torch()
        if self.d_tau is None:
            raise ValueError("%s() needs a listener built by for_slots" % who)
        if d_offsets.dtype != torch.int32 or not d_offsets.is_cuda or tuple(d_offsets.shape) != (self.B,) or not d_offsets.is_contiguous():
            raise ValueError("d_offsets must be a contiguous int32 cuda tensor [%d], got %s %s" % (self.B, d_offsets.dtype, tuple(d_offsets.shape)))
        return torch

    def retarget(self, d_offsets):
        """Re-design every beam for the slots of d_offsets, an int32 cuda tensor [slots] -- offsets[-1] of SourceTracker.update, a row
        of BeamListener.sources: enqueues bf_lcmv_design_device on the current stream, which writes self.d_taps IN PLACE (the address
        a captured graph reads stays valid).  -> (d_status int32 [slots], d_kept int32 [slots, K, slots]), the listener's own tensors."""
        self._check_slots("retarget", d_offsets)
        call("bf_lcmv_design_device", self.d_tau.data_ptr(), self.n_dirs, self.n, d_offsets.data_ptr(), self.B, self.offset_per_dir, self.T,
             int(self.bins[0]), int(self.bins[-1]), self.rho, self.d_gains.data_ptr(), self.d_taps.data_ptr(), self.d_kept.data_ptr(),
             self.d_status.data_ptr())
        self.taps = None
        return self.d_status, self.d_kept

    def _mvdr_args(self, loading, seg_hop, window):
        """What adapt and learn check and choose alike -> (loading, seg_hop, seg_first, segs, d_window or None)."""
        torch = _torch()
        N = config.N_SAMPLES
        loading, seg_hop = float(loading), int(seg_hop)
        if not (np.isfinite(loading) and loading > 0.0):
            raise ValueError("loading must be finite and > 0, got %g" % loading)
        if seg_hop < 1:
            raise ValueError("seg_hop must be >= 1, got %d" % seg_hop)
        seg_first = max(0, N - self.hop - self.T + 1) if self.hop > 0 else 0
        segs = (N - seg_first - self.T) // seg_hop + 1
        if window is None:
            return loading, seg_hop, seg_first, segs, None
        win = np.ascontiguousarray(window, dtype=np.float64)
        if win.shape != (self.T,):
            raise ValueError("window must be [n_taps = %d], got shape %s" % (self.T, win.shape))
        if self._window is None or not np.array_equal(self._window[0], win):
            self._window = (win.copy(), torch.from_numpy(win).to(self.device))
        return loading, seg_hop, seg_first, segs, self._window[1]

    def _mvdr_workspaces(self, P):
        """d_snap for P snapshots (kept until another count is asked for; P = 0: none needed), d_cov, d_chol and d_fallback once."""
        torch = _torch()
        K = int(self.bins.size)
        if self.d_cov is None:
            self.d_cov = torch.empty((K, self.n, self.n, 2), dtype=torch.float64, device=self.device)
            self.d_chol = torch.empty((K, self.n, self.n, 2), dtype=torch.float64, device=self.device)
            self.d_fallback = torch.zeros((K,), dtype=torch.int32, device=self.device)
        if P > 0 and self._mvdr_key != P:
            self.d_snap = torch.empty((P, K, self.n, 2), dtype=torch.float64, device=self.device)
            self._mvdr_key = P

    def adapt(self, d_frames, d_offsets, loading=0.1, seg_hop=16, window=None):
        """Re-design every beam from the covariance of d_frames (float32 cuda [F, M_total, N_SAMPLES], what `listen` takes) with unit
        response towards the slots of d_offsets (int32 cuda [slots], as `retarget`): enqueues bf_mvdr_design_device on the current
        stream -- design_mvdr_slots' design -- which writes self.d_taps IN PLACE, where retarget writes and listen reads.
        Segments of n_taps samples every seg_hop samples: of the whole window without a hop; with one, from max(0, N - hop - T + 1) on,
        so consecutive overlapping windows never count one segment twice.  window: float64 [n_taps] or None (rectangular).  The
        workspaces (d_snap, d_cov, d_chol) are allocated on the first call for a frame count and kept.
        -> (d_status int32 [slots], d_fallback int32 [K]: 1 where a bin fell back to the beam without nulls), the listener's own tensors."""
        self._check_slots("adapt", d_offsets)
        frames = self._frames(d_frames)
        F, m_total, N = frames.shape
        loading, seg_hop, seg_first, segs, d_window = self._mvdr_args(loading, seg_hop, window)
        self._mvdr_workspaces(F * segs)
        call("bf_mvdr_design_device", frames.data_ptr(), m_total, F, nat.iptr(self.mics), self.n, seg_first, seg_hop, segs,
             None if d_window is None else d_window.data_ptr(), self.d_tau.data_ptr(), self.n_dirs, d_offsets.data_ptr(), self.B, self.offset_per_dir,
             self.T, int(self.bins[0]), int(self.bins[-1]), loading, self.d_snap.data_ptr(), self.d_cov.data_ptr(), self.d_chol.data_ptr(),
             self.d_gains.data_ptr(), self.d_taps.data_ptr(), self.d_status.data_ptr(), self.d_fallback.data_ptr())
        self.taps = None
        return self.d_status, self.d_fallback

    def _mvdr_state(self):
        """d_acc, d_mass and d_used, allocated once (empty) and kept: the addresses a captured graph reads stay valid."""
        torch = _torch()
        if self.d_acc is None:
            self.d_acc = torch.zeros((int(self.bins.size), self.n, self.n, 2), dtype=torch.float64, device=self.device)
            self.d_mass = torch.zeros((1,), dtype=torch.float64, device=self.device)
            self.d_used = torch.zeros((2,), dtype=torch.int32, device=self.device)

    def _learn_call(self, frames_ptr, m_total, F, seg_first, seg_hop, segs, window_ptr, weights_ptr, forget, d_offsets, loading, snap_ptr):
        call("bf_mvdr_learn_device", frames_ptr, m_total, F, nat.iptr(self.mics), self.n, seg_first, seg_hop, segs, window_ptr, weights_ptr, forget,
             self.d_tau.data_ptr(), self.n_dirs, d_offsets.data_ptr(), self.B, self.offset_per_dir, self.T, int(self.bins[0]), int(self.bins[-1]), loading,
             self.d_acc.data_ptr(), self.d_mass.data_ptr(), self.d_used.data_ptr(), snap_ptr, self.d_cov.data_ptr(), self.d_chol.data_ptr(),
             self.d_gains.data_ptr(), self.d_taps.data_ptr(), self.d_status.data_ptr(), self.d_fallback.data_ptr())
        self.taps = None

    def learn(self, d_frames, d_offsets, weights=None, forget=1.0, loading=0.1, seg_hop=16, window=None):
        """`adapt` with a memory: the covariance is the listener's STATE (d_acc float64 [K, M, M, 2], d_mass float64 [1]), advanced by
        d_frames and kept for the next call; enqueues bf_mvdr_learn_device -- mvdr_learn then design_mvdr_learned on the host -- which
        writes self.d_taps in place.  weights: a float64 cuda tensor [F] or None (all 1); a frame is learned iff its weight is finite
        and > 0, so (match[:, s] < 0).double() of SourceTracker.update learns from the frames in which slot s was not heard, with no
        host round trip.  forget in (0, 1] multiplies the state once per LEARNED frame.  Segments, window and loading as `adapt`.
        A captured graph that holds this call advances the state with every replay.
        -> (d_status int32 [slots], d_fallback int32 [K], d_used int32 [2] = (frames learned, weights refused)), the listener's own tensors."""
        torch = self._check_slots("learn", d_offsets)
        frames = self._frames(d_frames)
        F, m_total, N = frames.shape
        loading, seg_hop, seg_first, segs, d_window = self._mvdr_args(loading, seg_hop, window)
        forget = float(forget)
        if not 0.0 < forget <= 1.0:
            raise ValueError("forget must be in (0, 1], got %g" % forget)
        if weights is not None and (weights.dtype != torch.float64 or not weights.is_cuda or tuple(weights.shape) != (F,) or not weights.is_contiguous()):
            raise ValueError("weights must be a contiguous float64 cuda tensor [%d], got %s %s" % (F, weights.dtype, tuple(weights.shape)))
        self._mvdr_workspaces(F * segs)
        self._mvdr_state()
        self._learn_call(frames.data_ptr(), m_total, F, seg_first, seg_hop, segs, None if d_window is None else d_window.data_ptr(),
                         None if weights is None else weights.data_ptr(), forget, d_offsets, loading, self.d_snap.data_ptr())
        return self.d_status, self.d_fallback, self.d_used

    def reaim(self, d_offsets, loading=0.1):
        """New taps for the slots of d_offsets from the state as it stands (bf_mvdr_learn_device with no frames): what to call when the
        tracker moves a slot.  The state is not changed; an empty state gives the beams without nulls and fallback 1 at every bin.
        -> (d_status int32 [slots], d_fallback int32 [K])."""
        self._check_slots("reaim", d_offsets)
        loading = self._mvdr_args(loading, 1, None)[0]
        self._mvdr_workspaces(0)
        self._mvdr_state()
        self._learn_call(None, int(self.mics.max()) + 1, 0, 0, 1, 1, None, None, 1.0, d_offsets, loading, None)
        return self.d_status, self.d_fallback

    def forget_all(self):
        """Empty the state: d_acc and d_mass are zeroed IN PLACE on the current stream."""
        self._mvdr_state()
        self.d_acc.zero_()
        self.d_mass.zero_()

    def taps_host(self):
        """The taps the beams read now, fetched from the device (synchronises): float32 [B, M, T], also kept as `.taps`."""
        self.taps = self.d_taps.cpu().numpy()
        return self.taps

    def listen(self, d_frames):
        """d_frames float32 cuda [F, M_total, N_SAMPLES] -> float32 [F, B, N_SAMPLES]; with a hop, frame f's history is frame f - 1,
        frame 0's the carried frame (silence without one).  Does not change the carried state."""
        torch = _torch()
        frames = self._frames(d_frames)
        F, m_total, N = frames.shape
        out = torch.empty((F, self.B, N), dtype=torch.float32, device=self.device)
        call("bf_filter_sum_device", frames.data_ptr(), m_total, F, self.hop, self._prev_ptr(), nat.iptr(self.mics), self.n, self.d_taps.data_ptr(),
             self.T, self.B, out.data_ptr(), N)
        return out
