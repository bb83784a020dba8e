"""The detector's convolutions (csrc/conv_kernels.hip): one table of the launch branches the tests want, and the shapes that reach them.

A BRANCH is what plan_conv2d decides and bf_plan_conv2d / bf_last_conv2d_plan report (include/beamformer_hip.h), without the grid:

    (element bytes, family, bm, bn, chunks per row, kCat, kSplit, fast_tap, wide store)

BRANCHES lists every such tuple that can come back with no environment switch set, under the two setters bf_conv2d_use_dma_kernel (0: the
register-staged kernel; 2: the patch kernel in float32 too) and bf_conv2d_f32_mode.  It is written out from the rules of the launch, not
asked of the planner: tests/test_conv_branches_host.py checks that the planner returns every one of them and nothing else.

A ROW is a branch plus the layer that must take it -- (C, N, window, stride, pad), where the sources of a 1x1 layer come from, whether the
output is a channel slice, a residual, a bias, SiLU.  Several rows may want the same branch (the 1x1 "virtual concatenation" kernels are
entered with one dense source, with two sources, and with an upsampled first source).  The layer is chosen so that the tile edges are
live: N is never a multiple of bn, N is a multiple of the 16-byte chunk exactly where the wide store epilogue is wanted, and the shape --
found by find_shape below, never written here -- has more than one row of tiles with a ragged last one.

find_shape walks LADDER, a fixed list of (B, H, W) in increasing pixel count, asks bf_plan_conv2d at the given number of compute units and
takes the first shape whose plan is the row's branch, inside the caps: every operand tensor at most 32 MiB, M * N * K at most 2e9 (the
float64 reference then takes a second or two).  The tile picker's choice depends on M / (compute units) through a ceiling, so which shape
that is differs from device to device; a 64 x 128 tile wins only in windows one 64-pixel tile wide, hence the density of the ladder."""
import collections
import ctypes as C

F16, F32 = 2, 4
REG, DMA, PATCH = 0, 1, 2
FAMILY = {REG: "reg", DMA: "dma", PATCH: "patch"}
TILES = [(128, 128), (128, 64), (64, 128), (64, 64), (128, 32)]

Branch = collections.namedtuple("Branch", "eb family bm bn cpr cat split fast_tap wide")


def _branches():
    out = []
    for eb in (F16, F32):
        for wide in (1, 0):
            for bn in (32, 64, 128):                      # the register-staged kernel: 128-pixel tiles, three channel widths x kCat
                for cat in (0, 1):
                    out.append(Branch(eb, REG, 128, bn, 4, cat, 0, 0, wide))
            out.append(Branch(eb, PATCH, 128, 32, 0, 0, 0, 0, wide))
            for split in ((0,) if eb == F16 else (0, 1)):
                for bm, bn in TILES:
                    # 128-byte rows: float16 layers of 128 channels and more, so never the 32-channel tile; never with the split
                    for cpr in ((4, 8) if eb == F16 and bn >= 64 else (4,)):
                        out.append(Branch(eb, DMA, bm, bn, cpr, 1, split, 0, wide))
                        for fast_tap in (0, 1):           # the window path (fast_tap never comes with kCat)
                            out.append(Branch(eb, DMA, bm, bn, cpr, 0, split, fast_tap, wide))
    return out


BRANCHES = _branches()


def settings(branch):
    """(bf_conv2d_use_dma_kernel, bf_conv2d_f32_mode) under which the branch is asked for."""
    if branch.family == REG:
        return 0, 0
    if branch.family == PATCH:
        return (1 if branch.eb == F16 else 2), 0
    return 1, branch.split


class Row(object):
    """branch: the tuple wanted.  c, n, k (one number or (kh, kw)), stride, pad: the layer.  src: None (a window layer), or how a 1x1 layer's input arrives --
    "dense" (one tensor of c channels), "two" (channels [0, c1) from a slice of one buffer, [c1, c) from a slice of another), "up" (as "two",
    the first source at half the size, read through a nearest 2x upsampling).  dma: the bf_conv2d_use_dma_kernel setting (settings() unless
    the row shows a layer that leaves the LDS-DMA kernel by itself).  sliced: the output is a channel slice (ldy > n)."""

    def __init__(self, branch, c, n, k, stride, pad, src=None, c1=0, dma=None, note=""):
        self.branch, self.c, self.n, self.stride, self.pad, self.src, self.c1, self.note = branch, c, n, stride, pad, src, c1 or c, note
        self.kh, self.kw = k if isinstance(k, tuple) else (k, k)
        self.dma, self.mode = settings(branch)
        if dma is not None:
            self.dma = dma
        self.index = self.sliced = self.residual = self.bias = self.silu = None      # (set by _rows)

    @property
    def E(self):
        return 16 // self.branch.eb

    @property
    def K(self):
        return self.kh * self.kw * self.c

    @property
    def ldy(self):
        # guard channels: a whole chunk where the wide epilogue is wanted, an odd count otherwise
        return self.n + ((self.E if self.branch.wide else 3) if self.sliced else 0)

    @property
    def ld1(self):
        return self.c1 + (self.E if self.src in ("two", "up") else 0)

    @property
    def ld2(self):
        return (self.c - self.c1 + 2 * self.E) if self.src in ("two", "up") else 0

    @property
    def id(self):
        b = self.branch
        return "%03d-%s-%s-%dx%d-r%d%s%s%s-%s%s" % (self.index, "f16" if b.eb == F16 else "f32", FAMILY[b.family], b.bm, b.bn, 16 * b.cpr, "-cat" if b.cat else "",
                                                  "-split" if b.split else "", "-tap" if b.fast_tap else "", "wide" if b.wide else "scalar",
                                                  ("-" + self.src if self.src else "") + ("-" + self.note if self.note else ""))

    def out_hw(self, h, w):
        return (h + 2 * self.pad - self.kh) // self.stride + 1, (w + 2 * self.pad - self.kw) // self.stride + 1


def _n_for(b):
    """Output channels: inside the branch's tile width, never a multiple of it, a multiple of the 16-byte chunk (8 float16 / 4 float32) exactly
    where the wide epilogue is wanted.  (64 x 128 tiles win with three columns of 128 channels against six of 64; 128-byte rows need 128 channels and more.)"""
    if b.bn == 32:
        return 24 if b.wide else 18
    if (b.bm, b.bn) == (64, 128) and b.family == DMA:
        return 328 if b.wide else 323
    if b.bn == 64 and b.cpr != 8:
        return 72 if b.wide else 70
    return 200 if b.wide else 197


def _rows():
    rows = []
    for b in BRANCHES:
        E, n = 16 // b.eb, _n_for(b)
        small = b.bm * b.bn <= 4096
        if b.family == PATCH:                             # the stem: 4 channels under a 6 x 6 window
            rows.append(Row(b, 4, n, 6, 2, 2))
        elif b.family == REG and not b.cat:
            rows.append(Row(b, 4 * E, n, 3, 2, 1))
        elif b.family == REG:
            rows.append(Row(b, 64, n, 1, 1, 0, "dense"))
            # two sources that do not meet on a 64-byte stage edge leave the LDS-DMA kernel by themselves: asked for with the switch at 1
            rows.append(Row(b, 64, n, 1, 1, 0, "two", c1=3 * E, dma=1, note="c1-off-stage"))
        elif b.cat:
            c = 512 if b.cpr == 8 else 64                 # 128-byte rows: 1x1 layers with K >= 512
            stage = b.cpr * E                             # elements of K per staged row: the two sources meet on a stage edge
            rows.append(Row(b, c, n, 1, 1, 0, "dense"))
            rows.append(Row(b, c, n, 1, 1, 0, "two", c1=stage, note="c1-on-stage"))
            rows.append(Row(b, c, n, 1, 1, 0, "up", c1=c - stage))
            if b.eb == F16 and b.cpr == 4 and b.bn >= 64:
                # K = 512 and 128+ channels would take 128-byte rows; a first source of 96 channels (not whole 128-byte stages) must drop them
                rows.append(Row(b, 512, n if n >= 128 else (200 if b.wide else 197), 1, 1, 0, "two", c1=12 * E, note="c1-off-row"))
        elif b.cpr == 8:
            if b.fast_tap:                                # K = 4 * 4 * 64 = 1024, a tap is one whole 128-byte stage
                rows.append(Row(b, 64, n, 4, 1, 1))
            else:                                         # K = 1 * 16 * 32 = 512 under one window row: a tap is half a 128-byte stage
                rows.append(Row(b, 32, n, (1, 16), 1, 0, note="c-short"))
        elif b.fast_tap:
            rows.append(Row(b, 4 * E, n, 3, 2 if small else 1, 1))
        elif b.wide:                                      # fast_tap off: fewer than four chunks of channels ...
            rows.append(Row(b, 2 * E, n, 3, 2 if small else 1, 1, note="c-short"))
        else:                                             # ... or more than 32 taps
            rows.append(Row(b, 8, n, 6, 1, 2, note="taps-36"))
    for i, r in enumerate(rows):
        r.index = i
        r.sliced, r.residual = i % 2 == 0, (i // 2) % 2 == 0
        r.bias, r.silu = i % 5 != 0, i % 3 != 0
        if r.branch.family == PATCH:                      # (four rows: the counters alone would give them all a bias)
            r.bias = bool(r.branch.wide)
    return rows


ROWS = _rows()

_SIDES = [5, 7, 10, 12, 14, 17, 20, 23, 26, 29, 34, 38, 41, 46, 50, 52, 53, 54, 56, 58, 61, 62, 66, 70, 72, 73, 74, 75, 78, 82, 86, 89, 90, 92, 94, 97, 102, 104, 106,
          110, 113, 118, 122, 126, 131]
LADDER = sorted(((b, h, w) for b in (1, 2, 3) for i, h in enumerate(_SIDES) for w in _SIDES[i:]), key=lambda s: (s[0] * s[1] * s[2], s))

MAX_OPERAND_BYTES = 32 << 20
MAX_MNK = 2 * 10 ** 9
OUT_LEN = 16


def plan(lib, row, B, H, W, n_cus, y_misaligned=False):
    """bf_plan_conv2d of the row's layer at [B, H, W] output-side pixels of a 1x1 layer / input pixels of a window layer -> (rc, list of 16)"""
    out = (C.c_longlong * OUT_LEN)(*([-7] * OUT_LEN))
    cat = row.src in ("two", "up")
    rc = lib.bf_plan_conv2d(row.branch.eb, B, H, W, row.c, row.n, row.kh, row.kw, row.stride, row.pad, row.ldy, int(row.residual), row.n if row.residual else 0,
                            row.c1 if cat else row.c, row.ld1 if cat else row.c, int(row.src == "up"), int(cat), row.ld2, 8 if y_misaligned else 0,
                            row.dma, row.mode, n_cus, out)
    return rc, list(out)


def branch_of(eb_and_plan):
    return Branch(*eb_and_plan[:9])


def in_caps(row, B, H, W):
    eb, (ho, wo) = row.branch.eb, row.out_hw(H, W)
    if ho < 1 or wo < 1:
        return False
    m = B * ho * wo
    x_bytes = B * H * W * max(row.c, row.ld2, row.ld1) * eb
    y_bytes = (m + 2 * wo) * row.ldy * eb
    w_bytes = row.n * (row.K + 128) * eb
    return max(x_bytes, y_bytes, w_bytes) <= MAX_OPERAND_BYTES and m * row.n * row.K <= MAX_MNK


def find_shape(lib, row, n_cus):
    """The first (B, H, W) of the ladder whose plan is the row's branch, with at least two rows of tiles and a ragged last one, inside the
    caps -> ((B, H, W), plan) or None."""
    for B, H, W in LADDER:
        if (row.src == "up" or row.c < row.E) and (H % 2 or W % 2):       # an upsampled source; float16 with 4 channels: even sizes
            continue
        if not in_caps(row, B, H, W):
            continue
        ho, wo = row.out_hw(H, W)
        m = B * ho * wo
        if m <= row.branch.bm or m % row.branch.bm == 0:
            continue
        rc, p = plan(lib, row, B, H, W, n_cus)
        if rc == 0 and branch_of(p) == row.branch:
            return (B, H, W), p
    return None
