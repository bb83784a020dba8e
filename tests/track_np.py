"""NumPy restatement of bf_track_sources_device (include/beamformer_hip.h): a plain-loop float32 reading of the definition, one
operation per line where the rounding matters.  Every float is an np.float32 scalar, so each +, -, *, / rounds once to float32 as
the kernel's does (the build contracts nothing).

  track(offsets, ...)   -> (track_offsets [F, slots], ids [F, slots], pos [F, slots, 4], match [F, slots], counts [F, 4], state)
  state_words(slots)    -> 4 + 12 * slots

`state` is an int32 array in the d_state word layout (floats stored by their bits); None or all zeros is a fresh stream.  The input
array is not modified; the returned one is new."""
import numpy as np

f32 = np.float32
MAX_SLOTS = 64
INT_SAFE = f32(2147483520.0)          # the largest float32 below 2^31


def state_words(slots):
    return 4 + 12 * slots if 1 <= slots <= MAX_SLOTS else -1


def scripted_scene(frames=40, k=4, rows=41, cols=23, offset_per_dir=3, flip=7, gap=(20, 24), alarms=((5, 35, 2), (26, 3, 20))):
    """The two-source scene the host and GPU tests share -> int32 [frames, k] offsets as bf_peaks_device would write them.
    Source A walks from (10, 5) one row down every 4 frames, source B stays at (30, 15); which of the two comes first flips every
    `flip` frames (two talkers of similar level); B is missing in frames [gap[0], gap[1]); each (frame, x, y) of `alarms` is a
    one-frame detection far from both, in the column after the sources; unused columns hold -1."""
    offs = np.full((frames, k), -1, dtype=np.int32)
    for f in range(frames):
        srcs = [(10 + f // 4, 5), (30, 15)]
        if gap[0] <= f < gap[1]:
            srcs = srcs[:1]
        if (f // flip) % 2 and len(srcs) == 2:
            srcs.reverse()
        srcs += [(ax, ay) for af, ax, ay in alarms if af == f]
        for j, (sx, sy) in enumerate(srcs):
            offs[f, j] = (sx * cols + sy) * offset_per_dir
    return offs


def _pixel(v, n):
    """clamp((int)rintf(v), 0, n - 1); the clamp to the int range happens in float so that no conversion overflows (NaN -> 0)."""
    r = np.rint(f32(v))
    if not r >= 0:
        return 0
    return min(int(min(r, INT_SAFE)), n - 1)


def track(offsets, rows, cols, offset_per_dir, slots, gate=3.0, max_miss=5, min_hits=3, q=0.1, r=0.1, state=None):
    offsets = np.asarray(offsets, dtype=np.int32)
    F, k = offsets.shape
    assert 1 <= slots <= MAX_SLOTS and 1 <= k <= 64
    q, r = f32(q), f32(r)
    gate2 = f32(gate) * f32(gate)
    D = rows * cols
    words = np.zeros(state_words(slots), dtype=np.int32) if state is None else np.array(state, dtype=np.int32).ravel()
    assert words.size == state_words(slots)
    fw = words.view(np.float32)
    next_id = int(words[0])
    tid = [int(words[4 + 12 * s]) for s in range(slots)]
    hits = [int(words[5 + 12 * s]) for s in range(slots)]
    miss = [int(words[6 + 12 * s]) for s in range(slots)]
    x, vx, y, vy, p00, p01, p11 = ([f32(fw[4 + 12 * s + 4 + i]) for s in range(slots)] for i in range(7))

    t_off = np.full((F, slots), -1, dtype=np.int32)
    t_ids = np.zeros((F, slots), dtype=np.int32)
    t_pos = np.zeros((F, slots, 4), dtype=np.float32)
    t_match = np.full((F, slots), -1, dtype=np.int32)
    counts = np.zeros((F, 4), dtype=np.int32)

    for f in range(F):
        # the frame's detections: column -> (zx, zy)
        det = {}
        for j in range(k):
            o = int(offsets[f, j])
            if o >= 0 and o % offset_per_dir == 0 and o // offset_per_dir < D:
                d = o // offset_per_dir
                det[j] = (f32(d // cols), f32(d % cols))
        invalid = k - len(det)
        live = [s for s in range(slots) if tid[s] != 0]
        # 1. predict
        for s in live:
            x[s] = x[s] + vx[s]
            y[s] = y[s] + vy[s]
            a = p00[s] + p01[s]
            b = p01[s] + p11[s]
            p00[s] = (a + b) + q
            p01[s] = b
            p11[s] = p11[s] + q
        # 2. associate: the smallest (cost, slot, column) among eligible pairs with both ends free, until none is left
        pairs = []
        for s in live:
            for j, (zx, zy) in det.items():
                dx = zx - x[s]
                dy = zy - y[s]
                cost = dx * dx + dy * dy
                if cost <= gate2:
                    pairs.append((float(cost), s, j))
        pairs.sort()
        taken_s, taken_j = {}, set()
        for _, s, j in pairs:
            if s not in taken_s and j not in taken_j:
                taken_s[s] = j
                taken_j.add(j)
        born = ended = dropped = 0
        for s in live:
            if s in taken_s:
                # 3. update
                zx, zy = det[taken_s[s]]
                S = p00[s] + r
                k0 = p00[s] / S
                k1 = p01[s] / S
                e = zx - x[s]
                x[s] = x[s] + k0 * e
                vx[s] = vx[s] + k1 * e
                e = zy - y[s]
                y[s] = y[s] + k0 * e
                vy[s] = vy[s] + k1 * e
                o00, o01, o11 = p00[s], p01[s], p11[s]
                p00[s] = o00 - k0 * o00
                p01[s] = o01 - k0 * o01
                p11[s] = o11 - k1 * o01
                hits[s] = hits[s] + 1
                miss[s] = 0
                t_match[f, s] = taken_s[s]
            else:
                # 4. coast
                miss[s] = miss[s] + 1
                if miss[s] > max_miss:
                    tid[s] = 0
                    ended += 1
        # 5. birth
        for j in sorted(det):
            if j in taken_j:
                continue
            free = [s for s in range(slots) if tid[s] == 0]
            if not free:
                dropped += 1
                continue
            s = free[0]
            next_id += 1
            tid[s], hits[s], miss[s] = next_id, 1, 0
            x[s], y[s] = det[j]
            vx[s] = vy[s] = f32(0)
            p00[s], p01[s], p11[s] = f32(1), f32(0), f32(1)
            t_match[f, s] = j
            born += 1
        # 6. write
        for s in range(slots):
            if tid[s] == 0:
                continue
            t_ids[f, s] = tid[s]
            t_pos[f, s] = (x[s], y[s], vx[s], vy[s])
            if hits[s] >= min_hits:
                t_off[f, s] = (_pixel(x[s], rows) * cols + _pixel(y[s], cols)) * offset_per_dir
        counts[f] = (born, ended, dropped, invalid)

    out = np.zeros_like(words)
    fo = out.view(np.float32)
    out[0] = next_id
    for s in range(slots):
        b = 4 + 12 * s
        if tid[s] == 0:
            continue                      # a free slot is stored as zeros
        out[b:b + 3] = (tid[s], hits[s], miss[s])
        fo[b + 4:b + 11] = (x[s], vx[s], y[s], vy[s], p00[s], p01[s], p11[s])
    return t_off, t_ids, t_pos, t_match, counts, out
