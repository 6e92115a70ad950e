"""Case builders and path predicates for tests/test_roi_align_stress.py: RoIAlign (csrc/roi_align.hip) away from the one
point the rest of the suite runs it at (7 x 7, adaptive sampling, aligned, C in {8, 64, 256, 512, 2048}).  CPU only, imports
without a GPU.

The launcher and the kernels choose between their paths with a dozen decisions; the functions below restate each one as a
plain function of the fp64 geometry (head_audit.roi_setup) and the map shapes, with the constants named as in the source:

  * forward: a RoI leaves the rows form for the per-sample form when PH > RB_MAXP, PW > 7 (the seven column accumulators),
    its batch index is bad, or one of its weight tables overflows: a bin whose samples reach FR_SPAN pixels past the first one
    (``hi - o >= FR_SPAN``);
  * atomic backward (fp32 maps, or bf16 with a pooled side above RB_MAXP): the per-sample scatter when PH or PW > RB_MAXP or
    a table overflows at RB_SPAN;
  * tile backward (bf16, PH and PW <= RB_MAXP): tiles per workgroup = tiles * channel chunks / 2048 clamped to 1 .. TPW, a
    ragged last workgroup per image when the tiles of an image are no multiple of it, the tile-by-tile walk for a
    (level, image) group of more than TB_THREADS RoIs, a second 4 x 4 bin block when more than four bin rows or columns of a
    RoI carry weight on one tile, ``chan_ok`` for a last 64-channel wave that is not full, channel chunks on blockIdx.y;
  * processing order: one launch (roi_order_rank_kernel) up to 8192 RoIs, the key kernel and a host-side sort above.

A case holds its RoIs, its maps' shapes and the predicates it exists for; ``Case.check()`` asserts them, and that no RoI that
defines a path is borderline (head_audit's ``near``: within fp32 rounding of a discrete choice, where the auditor would accept
either side).  Zero-area RoIs are borderline by construction - ceil(0) sits on its threshold - and exempt: their fp32 extent
is exactly 0, so the kernel takes the fp64 side, which the GPU tests assert through ``roi_other_side == 0``.
"""
import functools

import torch

import head_audit as HA

FR_SPAN = 32
RB_SPAN = 96
RB_MAXP = 8
FR_MAXPW = 7                 # the rows forward's column accumulators
TILE = 8
TPW = 8
TB_THREADS = 512
TPW_TILES = 2048             # tpw = tiles * chunks / 2048
ORDER_ONE_LAUNCH = 8192      # oadg_roi_order's limit
CHUNK = 256                  # channels per blockIdx.y
WAVE_CHANNELS = 64

F32, BF16 = torch.float32, torch.bfloat16
FWD = {F32: 'roi_align_fwd_rows_kernel<float>', BF16: 'roi_align_fwd_rows_kernel<unsigned short>'}
PYRAMID = ((32, 40), (16, 20), (8, 10))          # a 160 x 128 image at strides 4, 8, 16
IMAGE = (160, 128)


# ------------------------------------------------------------------------------------------------ geometry, per axis
def axis_coords(start, binsz, grid, P):
    """([n, P, G] sample coordinates start + p bin + (i + 0.5) bin / grid, i < grid mask)"""
    G = max(int(grid.max()), 1) if grid.numel() else 1
    i = torch.arange(G, dtype=torch.float64).view(1, 1, G)
    p = torch.arange(P, dtype=torch.float64).view(1, P, 1)
    g = grid.clamp_min(1).to(torch.float64).view(-1, 1, 1)
    b = binsz.view(-1, 1, 1)
    c = start.view(-1, 1, 1) + p * b + (i + 0.5) * b / g
    return c, (i < grid.view(-1, 1, 1)).expand_as(c)


def axis_pixels(c, valid, size):
    """the per-axis half of make_sample: (low, high, w_low, w_high, inside) of every sample coordinate"""
    s = size.view(-1, 1, 1)
    inside = valid & ~((c < -1.0) | (c > s.to(torch.float64)))
    c = torch.where(inside, c, torch.zeros_like(c)).clamp_min(0.0)
    lo = c.floor().long()
    edge = lo >= s - 1
    lo = torch.where(edge, (s - 1).expand_as(lo), lo)
    hi = torch.where(edge, lo, lo + 1)
    c = torch.where(edge, lo.to(torch.float64), c)
    l = c - lo.to(torch.float64)
    return lo, hi, 1.0 - l, l, inside


def axis_span(start, binsz, grid, P, size):
    """[n] the widest ``hi - o`` of axis_table over the RoI's bins (o: low pixel of the bin's first inside sample, hi: high
    pixel of its last one); -1 for a RoI without an inside sample.  Bins are not negative here (samples ascend)."""
    c, valid = axis_coords(start, binsz, grid, P)
    lo, hi, _, _, inside = axis_pixels(c, valid, size)
    big = torch.full_like(lo, 1 << 40)
    first = torch.where(inside, lo, big).amin(2)
    last = torch.where(inside, hi, -torch.ones_like(hi)).amax(2)
    return torch.where(last >= 0, last - first, -torch.ones_like(last)).amax(1)


def axis_weights(start, binsz, grid, P, size):
    """[n, P, max size] fp64 weight each bin puts on each pixel of its axis (the tables of the backward kernels)"""
    c, valid = axis_coords(start, binsz, grid, P)
    lo, hi, wl, wh, inside = axis_pixels(c, valid, size)
    W = torch.zeros((start.numel(), P, int(size.max()) if size.numel() else 1), dtype=torch.float64)
    m = inside.to(torch.float64)
    W.scatter_add_(2, lo, wl * m)
    W.scatter_add_(2, hi, wh * m)
    return W


def tile_bin_range(W):
    """[n, tiles] phi - plo of roi_align_bwd_tiles_kernel: the range of bins with a non-zero weight on each 8-pixel tile"""
    n, P, S = W.shape
    T = (S + TILE - 1) // TILE
    Wp = torch.zeros((n, P, T * TILE), dtype=W.dtype)
    Wp[:, :, :S] = W
    nz = Wp.view(n, P, T, TILE).abs().sum(3) > 0
    idx = torch.arange(P).view(1, P, 1)
    lo = torch.where(nz, idx, torch.full_like(idx, P)).amin(1)
    hi = torch.where(nz, idx + 1, torch.zeros_like(idx)).amax(1)
    return (hi - lo).clamp_min(0)


# ------------------------------------------------------------------------------------------------------------ cases
class Case:
    """RoIs [K, 5] fp32 on maps ``sizes`` ([N, C, H_l, W_l]) with the RoIAlign parameters; ``path``: the RoIs that define the
    case's path (all by default) - none of them may be borderline unless its area is zero"""

    def __init__(self, name, sizes, rois, PH=7, PW=7, sr=0, aligned=True, N=2, C=8, scales=None, finest=8, dtypes=(F32, BF16),
                 path=None):
        self.name = name
        self.shapes = [(N, C, h, w) for h, w in sizes]
        self.N, self.C, self.PH, self.PW, self.sr, self.aligned, self.finest = N, C, PH, PW, sr, aligned, finest
        self.scales = tuple(scales) if scales is not None else tuple(2.0 ** -(2 + l) for l in range(len(sizes)))
        self.rois = rois.to(torch.float32).reshape(-1, 5)
        self.K = self.rois.shape[0]
        self.dtypes = tuple(dtypes)
        self.path = torch.ones(self.K, dtype=torch.bool) if path is None else path
        self.claims = []             # (what, zero-argument predicate)

    def __repr__(self):
        return self.name

    def claim(self, what, fn):
        self.claims.append((what, fn))
        return self

    # -- fp64 geometry
    @functools.cached_property
    def setup(self):
        return HA.roi_setup(self.rois, self.shapes, self.scales, self.finest, self.PH, self.PW, self.sr, self.aligned)

    @property
    def lvl(self):
        return self.setup[0]

    @property
    def geo(self):
        return self.setup[1]

    @property
    def near(self):
        return self.setup[2]

    @functools.cached_property
    def zero_area(self):
        r = self.rois
        return (r[:, 3] == r[:, 1]) | (r[:, 4] == r[:, 2])

    @functools.cached_property
    def bad_batch(self):
        return (self.geo['batch'] < 0) | (self.geo['batch'] >= self.N)

    @functools.cached_property
    def spans(self):
        g = self.geo
        return (axis_span(g['sh'], g['bh'], g['gh'], self.PH, g['H']), axis_span(g['sw'], g['bw'], g['gw'], self.PW, g['W']))

    def coords(self, axis):
        g = self.geo
        s, b, n, P = (g['sh'], g['bh'], g['gh'], self.PH) if axis == 'y' else (g['sw'], g['bw'], g['gw'], self.PW)
        return axis_coords(s, b, n, P)

    def weights(self, axis):
        g = self.geo
        if axis == 'y':
            return axis_weights(g['sh'], g['bh'], g['gh'], self.PH, g['H'])
        return axis_weights(g['sw'], g['bw'], g['gw'], self.PW, g['W'])

    @functools.cached_property
    def samples_per_bin(self):
        return self.geo['gh'].clamp_min(0) * self.geo['gw'].clamp_min(0)

    @functools.cached_property
    def no_sample(self):
        """RoIs that reach no map element: bad batch, no samples, or every sample of one axis outside the map"""
        sy, sx = self.spans
        return self.bad_batch | (sy < 0) | (sx < 0)

    # -- the launcher's and the kernels' decisions
    @functools.cached_property
    def fwd_per_sample(self):
        """[K] RoIs the rows forward hands to roi_fwd_samples"""
        sy, sx = self.spans
        whole = self.PH > RB_MAXP or self.PW > FR_MAXPW
        return self.bad_batch | (sy >= FR_SPAN) | (sx >= FR_SPAN) | torch.full((self.K,), whole, dtype=torch.bool)

    @functools.cached_property
    def bwd_scatter(self):
        """[K] RoIs the atomic backward hands to roi_bwd_scatter"""
        sy, sx = self.spans
        whole = self.PH > RB_MAXP or self.PW > RB_MAXP
        return ~self.bad_batch & ((sy >= RB_SPAN) | (sx >= RB_SPAN) | torch.full((self.K,), whole, dtype=torch.bool))

    def tiles(self, dt):
        return dt == BF16 and self.PH <= RB_MAXP and self.PW <= RB_MAXP and self.K > 0

    def ordered(self, dt):
        return self.K >= 512 or self.tiles(dt)

    def kernels(self, dt):
        """the set head_audit.Auditor.kernels must hold after one forward + backward"""
        ks = {FWD[dt]}
        if self.ordered(dt):
            ks.add('roi_order_rank_kernel' if self.K <= ORDER_ONE_LAUNCH else 'roi_order_key_kernel')
        ks |= {'roi_align_bwd_tiles_kernel', 'roi_tile_box_kernel'} if self.tiles(dt) else {'roi_align_bwd_kernel'}
        return ks

    @property
    def chunks(self):
        return (self.C + CHUNK - 1) // CHUNK

    @property
    def tiles_per_image(self):
        return [((h + TILE - 1) // TILE) * ((w + TILE - 1) // TILE) for _, _, h, w in self.shapes]

    @property
    def tpw(self):
        t = self.N * sum(self.tiles_per_image) * self.chunks // TPW_TILES
        return min(max(t, 1), TPW)

    @functools.cached_property
    def group_sizes(self):
        """RoIs per (level, image) group of the processing order (the key's level and clamped batch index)"""
        grp = HA.roi_order_expect(self.rois, self.N, len(self.shapes), self.finest)[0][1]
        return torch.bincount(grp, minlength=len(self.shapes) * self.N)

    @functools.cached_property
    def second_block(self):
        """[K] RoIs with more than four bin rows or columns of non-zero weight on one tile they reach"""
        ry, rx = tile_bin_range(self.weights('y')), tile_bin_range(self.weights('x'))
        return ~self.bad_batch & (((ry > 4).any(1) & (rx > 0).any(1)) | ((rx > 4).any(1) & (ry > 0).any(1)))

    def on_last_tile(self, n, l=0):
        """whether a RoI of image ``n`` puts weight on the last tile of level ``l``"""
        _, _, h, w = self.shapes[l]
        m = (self.lvl == l) & (self.geo['batch'] == n)
        if not bool(m.any()):
            return False
        wy, wx = self.weights('y')[m], self.weights('x')[m]
        y0, x0 = (h - 1) // TILE * TILE, (w - 1) // TILE * TILE
        return bool(((wy[:, :, y0:h].sum((1, 2)) > 0) & (wx[:, :, x0:w].sum((1, 2)) > 0)).any())

    # -- operands
    def feats(self, dt, dev, seed=0):
        g = torch.Generator().manual_seed(1000 + seed)
        return [torch.randn(s, generator=g).to(dev, dt).contiguous(memory_format=torch.channels_last).requires_grad_(True)
                for s in self.shapes]

    def gout(self, dt, dev, seed=0):
        g = torch.Generator().manual_seed(2000 + seed)
        return torch.randn((self.K, self.C, self.PH, self.PW), generator=g).to(dev, dt)

    def check(self):
        bad = self.near & self.path & ~self.zero_area
        assert not bool(bad.any()), (self.name, 'borderline path RoIs', bad.nonzero().view(-1).tolist()[:8])
        c = self.rois[:, 1:][~torch.isnan(self.rois[:, 1:])]
        assert c.numel() == 0 or float(c.abs().max()) * max(self.scales) < 2 ** 11, self.name
        assert self.C >= 4 and self.C % 4 == 0, self.name
        for what, fn in self.claims:
            assert fn(), (self.name, what)
        return self


def rand_rois(K, seed, N=2, W=IMAGE[0], H=IMAGE[1], lo=4, hi=120, x0=-4.0, y0=-4.0):
    g = torch.Generator().manual_seed(seed)
    x1 = torch.rand(K, generator=g) * W * 0.8 + x0
    y1 = torch.rand(K, generator=g) * H * 0.8 + y0
    w = lo + torch.rand(K, generator=g) * (hi - lo)
    h = lo + torch.rand(K, generator=g) * (hi - lo)
    b = torch.randint(0, N, (K,), generator=g).float()
    return torch.stack([b, x1, y1, x1 + w, y1 + h], 1)


def settle(case, seed=0, only=None):
    """nudge the borderline RoIs (of ``only``, default all) by a fraction of a pixel until none is left"""
    g = torch.Generator().manual_seed(77 + seed)
    for _ in range(40):
        m = case.near & ~case.zero_area
        if only is not None:
            m = m & only
        if not bool(m.any()):
            return case
        rois = case.rois.clone()
        n = int(m.sum())
        rois[m, 1:] += (torch.rand((n, 4), generator=g) - 0.5) * 0.7
        case.rois = rois
        for k in ('setup', 'zero_area', 'bad_batch', 'spans', 'samples_per_bin', 'no_sample', 'fwd_per_sample', 'bwd_scatter',
                  'group_sizes', 'second_block'):
            case.__dict__.pop(k, None)
    raise AssertionError('%s: borderline RoIs left' % case.name)


def _levels_reached(c, n):
    return lambda: len(set(c.lvl[~c.bad_batch].tolist())) == n


# ---- 1. pooled shapes
POOLED = ((1, 1), (2, 7), (7, 2), (5, 7), (7, 8), (8, 7), (8, 8), (3, 8), (9, 4), (14, 14))


@functools.lru_cache(maxsize=None)
def pooled_case(PH, PW):
    c = settle(Case('pooled/%dx%d' % (PH, PW), PYRAMID, rand_rois(60, 21), PH=PH, PW=PW))
    c.claim('three levels', _levels_reached(c, 3))
    if PH > RB_MAXP or PW > RB_MAXP:
        c.claim('forward per sample', lambda: bool(c.fwd_per_sample.all()))
        c.claim('backward per-sample scatter', lambda: bool(c.bwd_scatter.all()))
        c.claim('bf16 leaves the tile kernel', lambda: not c.tiles(BF16) and 'roi_align_bwd_kernel' in c.kernels(BF16))
    elif PW > FR_MAXPW:
        c.claim('forward per sample inside the rows kernel', lambda: bool(c.fwd_per_sample.all()))
        c.claim('backward by tables', lambda: not bool(c.bwd_scatter.any()))
        c.claim('bf16 by tiles', lambda: c.tiles(BF16))
    else:
        c.claim('rows forward', lambda: not bool(c.fwd_per_sample.any()))
        c.claim('backward by tables', lambda: not bool(c.bwd_scatter.any()))
        c.claim('bf16 by tiles', lambda: c.tiles(BF16))
        if PH == 8:
            c.claim('two bin rows per wave', lambda: c.PH > 4 and c.PW <= FR_MAXPW)
    return c


@functools.lru_cache(maxsize=None)
def subpixel_case():
    """8 x 8 bins of RoIs smaller than a feature pixel: all 64 bins of a RoI on one tile - the tile kernel's second, third and
    fourth 4 x 4 block; some RoIs sit on a tile boundary (two tiles, eight bin rows each)"""
    g = torch.Generator().manual_seed(31)
    K = 48
    cx = torch.rand(K, generator=g) * 150 + 4
    cy = torch.rand(K, generator=g) * 118 + 4
    cx[:8] = torch.tensor([31.9, 32.1, 63.8, 64.3, 95.7, 96.2, 127.9, 31.8])       # 8-pixel tiles of level 0: 32 image px
    cy[:8] = torch.tensor([31.8, 64.1, 32.2, 95.9, 63.7, 31.9, 64.2, 96.1])
    w = 0.6 + torch.rand(K, generator=g) * 3.0                                     # below 4 image px = 1 feature pixel
    h = 0.6 + torch.rand(K, generator=g) * 3.0
    b = torch.randint(0, 2, (K,), generator=g).float()
    rois = torch.stack([b, cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
    c = settle(Case('pooled/8x8 subpixel', PYRAMID, rois, PH=8, PW=8))
    c.claim('smaller than a pixel', lambda: bool(((c.geo['bh'] * 8 < 1) & (c.geo['bw'] * 8 < 1)).all()))
    c.claim('second 4 x 4 block on every RoI', lambda: bool(c.second_block.all()))
    c.claim('bf16 by tiles', lambda: c.tiles(BF16))
    return c


# ---- 2. sampling parameters
def tiny_rois(K, seed, N=2):
    """RoIs narrower and lower than one feature pixel of level 0 (4 image px)"""
    g = torch.Generator().manual_seed(seed)
    x1 = torch.rand(K, generator=g) * 140 + 6
    y1 = torch.rand(K, generator=g) * 110 + 6
    w = 0.3 + torch.rand(K, generator=g) * 3.2
    h = 0.3 + torch.rand(K, generator=g) * 3.2
    return torch.stack([torch.randint(0, N, (K,), generator=g).float(), x1, y1, x1 + w, y1 + h], 1)


@functools.lru_cache(maxsize=None)
def sampling_case(sr, aligned):
    rois = torch.cat([rand_rois(40, 41), tiny_rois(16, 42)])
    tiny = torch.arange(56) >= 40
    c = settle(Case('sampling/sr%d %s' % (sr, 'aligned' if aligned else 'unaligned'), PYRAMID, rois, sr=sr, aligned=aligned))
    c.claim('fixed sample counts', lambda: bool(((c.geo['gh'] == sr) & (c.geo['gw'] == sr)).all()))
    c.claim('three levels', _levels_reached(c, 3))
    raw = c.rois.double()
    c.claim('RoIs below one pixel', lambda: bool(
        (((raw[:, 3] - raw[:, 1]) * 0.25 < 1) & ((raw[:, 4] - raw[:, 2]) * 0.25 < 1) & (c.lvl == 0))[tiny].all()))
    if not aligned:
        # max(rw, 1): the bins of the tiny RoIs are exactly 1 / P wide
        c.claim('the max(rw, 1) rule applies', lambda: bool(
            ((c.geo['bw'][tiny] == 1.0 / c.PW) & (c.geo['bh'][tiny] == 1.0 / c.PH)).all()))
    return c


WIDE_X, WIDE_Y, SQUARE = ((24, 800),), ((800, 24),), ((240, 240),)


def _strip_rois(bins, axis, thin, start=10.2, N=2):
    """stride-1 RoIs (aligned) with 7 bins of ``bins`` pixels along ``axis`` and 7 bins of ``thin`` pixels along the other"""
    rows = []
    for j, p in enumerate(bins):
        a0 = start + 0.5 + 1.3 * (j % 3)
        t0 = 3.3 + 0.5 + 0.9 * (j % 4)
        t = thin[j % len(thin)]
        a, tt = (a0, a0 + 7 * p), (t0, t0 + 7 * t)
        rows.append([j % N, a[0], tt[0], a[1], tt[1]] if axis == 'x' else [j % N, tt[0], a[0], tt[1], a[1]])
    return torch.tensor(rows, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def sparse_case(kind, axis):
    """sampling_ratio = 2 on wide bins: 'gaps' - bins of about 20 pixels, tables with zero-weight rows between the two
    samples; 'overflow' - bins of about 70 pixels, a two-sample bin that overflows FR_SPAN (and not RB_SPAN)"""
    bins = (19.3, 20.6, 21.7, 18.4) if kind == 'gaps' else (68.7, 70.3, 71.6, 66.9)
    c = Case('sampling/sr2 %s %s' % (kind, axis), WIDE_X if axis == 'x' else WIDE_Y, _strip_rois(bins, axis, (0.8, 1.6)),
             sr=2, scales=(1.0,))
    span = lambda: c.spans[1 if axis == 'x' else 0]      # noqa: E731
    if kind == 'gaps':
        def gaps():
            W = c.weights(axis)                          # [n, P, size]: zero entries strictly inside a bin's table
            nz = W > 0
            idx = torch.arange(W.shape[2]).view(1, 1, -1)
            lo = torch.where(nz, idx, torch.full_like(idx, 1 << 30)).amin(2)
            hi = torch.where(nz, idx, -torch.ones_like(idx)).amax(2)
            return bool(((hi - lo + 1) > nz.sum(2) + 4).all())
        c.claim('zero-weight rows between the samples', gaps)
        c.claim('rows forward', lambda: not bool(c.fwd_per_sample.any()))
    else:
        c.claim('two samples overflow FR_SPAN', lambda: bool(((span() >= FR_SPAN) & (span() < RB_SPAN)).all()))
        c.claim('forward per sample', lambda: bool(c.fwd_per_sample.all()))
    c.claim('backward by tables', lambda: not bool(c.bwd_scatter.any()))
    return c


# ---- 3. table thresholds
THRESHOLD_BINS = (31, 32, 33, 95, 96, 97)


@functools.lru_cache(maxsize=None)
def threshold_case(axis):
    """adaptive bins of p - 0.4 pixels (p samples, the widest bin spans p pixels) for p on both sides of FR_SPAN and RB_SPAN,
    one or two samples thin on the other axis (at most 194 samples per bin); 'xy': 33 x 33 on both axes"""
    if axis == 'xy':
        rois = torch.tensor([[0, 10.7, 6.9, 10.7 + 7 * 32.6, 6.9 + 7 * 32.6], [1, 4.9, 9.8, 4.9 + 7 * 31.7, 9.8 + 7 * 32.8]])
        c = Case('threshold/33 x 33', SQUARE, rois, scales=(1.0,))
        c.claim('both tables overflow FR_SPAN', lambda: bool(((c.spans[0] >= FR_SPAN) & (c.spans[1] >= FR_SPAN)).all()))
        c.claim('about 10^3 samples per bin', lambda: int(c.samples_per_bin.max()) <= 33 * 33)
        c.claim('backward by tables', lambda: not bool(c.bwd_scatter.any()))
        return c
    bins = [p - 0.4 for p in THRESHOLD_BINS] * 2
    c = Case('threshold/%s' % axis, WIDE_X if axis == 'x' else WIDE_Y, _strip_rois(bins, axis, (0.8, 1.6, 1.7)), scales=(1.0,))
    span = lambda: c.spans[1 if axis == 'x' else 0]      # noqa: E731
    c.claim('the widest bin spans p pixels', lambda: span().tolist() == list(THRESHOLD_BINS) * 2)
    c.claim('both sides of FR_SPAN', lambda: c.fwd_per_sample.tolist() == [p >= FR_SPAN for p in THRESHOLD_BINS] * 2)
    c.claim('both sides of RB_SPAN', lambda: c.bwd_scatter.tolist() == [p >= RB_SPAN for p in THRESHOLD_BINS] * 2)
    c.claim('thin on the other axis', lambda: int(c.samples_per_bin.max()) <= 2 * 97)
    c.claim('inside the map', lambda: not bool(c.no_sample.any()))
    return c


# ---- 4. channels
CHANNELS = (4, 8, 60, 68, 260, 264, 516)


@functools.lru_cache(maxsize=None)
def channel_case(C):
    c = settle(Case('channels/%d' % C, PYRAMID, rand_rois(40, 51), C=C))
    c.claim('three levels', _levels_reached(c, 3))
    c.claim('a partial 64-channel wave', lambda: C % WAVE_CHANNELS != 0)
    if C > CHUNK:
        c.claim('a narrow last chunk on blockIdx.y', lambda: c.chunks > 1 and C - (c.chunks - 1) * CHUNK in (4, 8))
    return c


# ---- 5. tiny and ragged maps
TINY_PYRAMID = ((9, 15), (5, 8), (3, 4), (1, 2))         # a 60 x 36 image at strides 4 .. 32
TINY_LEVELS = ((1, 1), (1, 9), (9, 1), (7, 8), (8, 8), (9, 9))


def _edge_rois(H, W):
    """stride-1, aligned (start = x1 - 0.5): the edge behaviours of one map, by name"""
    named = {
        'cover': [-1.83 - 0.5, -2.27 - 0.5, W + 1.41 + 0.5, H + 1.61 + 0.5],                    # hangs over every side
        'left': [-6.3, 0.2, -2.1, H - 0.3], 'right': [W + 2.2, 0.3, W + 6.4, H - 0.2],          # outside by more than a pixel
        'above': [0.2, -7.4, W - 0.3, -2.2], 'below': [0.3, H + 2.3, W - 0.2, H + 5.9],
        # first samples in (-1, 0]: start -0.9, a third of a pixel per bin (one sample per bin, at -0.9 + 0.17)
        'first': [-0.9 + 0.5, -0.9 + 0.5, -0.9 + 0.5 + 2.38, -0.9 + 0.5 + 2.38],
        # last samples between size - 1 and size
        'last': [W - 2.7 + 0.5, H - 2.7 + 0.5, W - 0.31 + 0.5, H - 0.31 + 0.5],
    }
    return named


@functools.lru_cache(maxsize=None)
def tiny_level_case(H, W):
    named = _edge_rois(H, W)
    names = list(named)
    rois = torch.tensor([[j % 2] + named[n] for j, n in enumerate(names)], dtype=torch.float64)
    c = Case('tiny/%dx%d' % (H, W), ((H, W),), rois, scales=(1.0,))
    k = {n: j for j, n in enumerate(names)}

    def inside(axis, j):
        cc, valid = c.coords(axis)
        size = (c.geo['H'] if axis == 'y' else c.geo['W'])[j]
        v = cc[j][valid[j]]
        return v, (v >= -1.0) & (v <= float(size))
    c.claim('covers the map and hangs over every side', lambda: all(
        bool((inside(a, k['cover'])[0] < -1).any()) and bool((inside(a, k['cover'])[0] > s).any())
        and bool(inside(a, k['cover'])[1].any()) for a, s in (('y', H), ('x', W))))
    for n, a in (('left', 'x'), ('right', 'x'), ('above', 'y'), ('below', 'y')):
        c.claim('%s: every sample outside' % n, lambda n=n, a=a: not bool(inside(a, k[n])[1].any()) and
                int(c.samples_per_bin[k[n]]) > 0 and bool(c.no_sample[k[n]]))
    c.claim('first samples in (-1, 0]', lambda: all(-1 < float(inside(a, k['first'])[0].min()) <= 0 for a in 'xy'))
    c.claim('last samples between size - 1 and size', lambda: all(
        s - 1 < float(inside(a, k['last'])[0].max()) < s for a, s in (('y', H), ('x', W))))
    return c


@functools.lru_cache(maxsize=None)
def tiny_pyramid_case():
    rois = torch.cat([rand_rois(70, 61, W=60, H=36, lo=1.5, hi=90, x0=-14.0, y0=-12.0),
                      torch.tensor([[0, -21.3, -17.8, 83.4, 55.9], [1, -3.1, -2.6, 62.7, 38.2]])])
    c = settle(Case('tiny/pyramid', TINY_PYRAMID, rois))
    c.claim('four levels', _levels_reached(c, 4))
    c.claim('RoIs wholly outside', lambda: bool((c.no_sample & ~c.bad_batch).any()))
    return c


# ---- 6. tiles per workgroup (bf16)
def _corner_rois(N, H, W, per_image, seed, lo=9.0, hi=40.0):
    """stride-1 RoIs on the last tiles of every image plus a few anywhere"""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for n in range(N):
        for j in range(per_image):
            w = lo + float(torch.rand(1, generator=g)) * (hi - lo)
            h = lo + float(torch.rand(1, generator=g)) * (hi - lo)
            if j % 3 == 2:
                x1 = float(torch.rand(1, generator=g)) * (W - w)
                y1 = float(torch.rand(1, generator=g)) * (H - h)
            else:                                         # ends within the last tile (or just past the map)
                x1 = W - w - 3.3 + float(torch.rand(1, generator=g)) * 5
                y1 = H - h - 3.3 + float(torch.rand(1, generator=g)) * 5
            rows.append([n, x1, y1, x1 + w, y1 + h])
    return torch.tensor(rows, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def tpw_case(kind):
    if kind == 'tpw5':
        N, H, C = 4, 408, 8
        rois = _corner_rois(N, H, H, 12, 71)
    elif kind == 'tpw2':
        N, H, C = 2, 264, 264
        rois = _corner_rois(N, H, H, 12, 72)
    else:
        # tpw8: image 0 holds more than 512 RoIs clustered on a few tiles (the last ones among them)
        N, H, C = 2, 728, 8
        g = torch.Generator().manual_seed(73)
        n0 = 560
        cx = torch.where(torch.arange(n0) % 2 == 0, torch.tensor(700.0), torch.tensor(40.0)) + torch.randn(n0, generator=g) * 6
        cy = torch.where(torch.arange(n0) % 2 == 0, torch.tensor(702.0), torch.tensor(330.0)) + torch.randn(n0, generator=g) * 6
        s = 8 + torch.rand(n0, generator=g) * 30
        rois = torch.cat([torch.stack([torch.zeros(n0), cx - s / 2, cy - s / 2, cx + s / 2, cy + s / 2], 1).double(),
                          _corner_rois(N, H, H, 6, 74)])
    want = {'tpw5': 5, 'tpw2': 2, 'tpw8': 8}[kind]
    c = settle(Case('tpw/%s' % kind, ((H, H),), rois, N=N, C=C, scales=(1.0,), dtypes=(BF16,)))
    c.claim('tiles per workgroup', lambda: c.tpw == want)
    c.claim('a ragged last workgroup', lambda: c.tiles_per_image[0] % c.tpw != 0)
    c.claim('RoIs on the last tile of every image', lambda: all(c.on_last_tile(n) for n in range(N)))
    if kind == 'tpw2':
        c.claim('two channel chunks, the second 8 wide', lambda: c.chunks == 2 and C - CHUNK == 8)
    if kind == 'tpw8':
        c.claim('a group of more than 512 RoIs', lambda: int(c.group_sizes.max()) > TB_THREADS)
    else:
        c.claim('groups of at most 512 RoIs', lambda: int(c.group_sizes.max()) <= TB_THREADS)
    return c


# ---- 7. batch indices and degenerate boxes
def degenerate_rois(N=2):
    nan = float('nan')
    named = [
        ('batch -1', [-1, 20.3, 18.7, 61.2, 50.9]), ('batch N', [N, 20.3, 18.7, 61.2, 50.9]),
        ('batch N + 5', [N + 5, 33.1, 12.2, 99.4, 80.6]),
        ('zero area, integer corners', [0, 40, 32, 40, 32]), ('zero area, fractional corners', [1, 40.3, 32.7, 40.3, 32.7]),
        ('zero width', [0, 52.6, 20.2, 52.6, 71.4]), ('zero height', [1, 12.9, 64.4, 88.1, 64.4]),
        ('inverted in x', [0, 90.2, 20.1, 41.7, 66.3]), ('inverted in y', [1, 30.4, 77.2, 80.9, 22.8]),
        ('inverted in x and y', [0, 120.6, 100.3, 31.9, 21.2]), ('inverted in x and y, small', [1, 50.3, 40.2, 44.1, 35.7]),
        ('NaN x1', [0, nan, 20.2, 60.4, 70.6]), ('NaN y2', [1, 18.3, 20.2, 60.4, nan]),
    ]
    return [n for n, _ in named], torch.tensor([r for _, r in named], dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def degenerate_case():
    names, deg = degenerate_rois()
    rois = torch.cat([rand_rois(24, 81), deg])
    c = Case('degenerate', PYRAMID, rois)
    c.degenerate = torch.arange(c.K) >= 24
    settle(c, only=~c.degenerate)
    c.names = names
    c.claim('no samples or a bad batch index', lambda: bool(
        (c.bad_batch | (c.geo['gh'] <= 0) | (c.geo['gw'] <= 0))[c.degenerate].all()))
    c.claim('the valid RoIs reach the maps', lambda: not bool(c.no_sample[~c.degenerate].any()))

    def both_inverted():
        # roi_level sees a positive product; the order key clamps the extents to 0: level 0
        k = 24 + names.index('inverted in x and y')
        return int(c.lvl[k]) > 0 and int(HA.roi_order_expect(c.rois, c.N, 3, c.finest)[0][1][k]) // c.N == 0
    c.claim('inverted on both axes: the forward level differs from the key level', both_inverted)
    return c


# ---- 8. more than 8192 RoIs
BIG_K = (8193, 9001)


@functools.lru_cache(maxsize=None)
def big_case(K):
    g = torch.Generator().manual_seed(91 + K)
    cx = torch.rand(K, generator=g) * 150 + 5
    cy = torch.rand(K, generator=g) * 118 + 5
    s = 3 + torch.rand(K, generator=g) ** 2 * 70                       # levels 0 .. 2, most on level 0
    a = 0.6 + torch.rand(K, generator=g) * 0.8
    b = torch.randint(0, 2, (K,), generator=g).float()
    rois = torch.stack([b, cx - s / 2, cy - s * a / 2, cx + s / 2, cy + s * a / 2], 1)
    c = settle(Case('big/%d' % K, PYRAMID, rois))
    c.claim('past the one-launch order', lambda: c.K > ORDER_ONE_LAUNCH)

    def ties():
        keys = HA.roi_order_expect(c.rois, c.N, 3, c.finest)[0][0]
        return int(torch.unique(keys).numel()) < 64 and c.K > 100 * int(torch.unique(keys).numel())
    c.claim('many RoIs per 64-pixel cell (tied keys)', ties)
    c.claim('three levels', _levels_reached(c, 3))
    c.claim('groups of more than 512 RoIs', lambda: int(c.group_sizes.max()) > TB_THREADS)
    return c


def all_cases():
    cs = [pooled_case(*p) for p in POOLED] + [subpixel_case()]
    cs += [sampling_case(sr, al) for sr in (1, 2, 3) for al in (True, False)]
    cs += [sparse_case(k, a) for k in ('gaps', 'overflow') for a in 'xy']
    cs += [threshold_case(a) for a in ('x', 'y', 'xy')]
    cs += [channel_case(C) for C in CHANNELS]
    cs += [tiny_level_case(*s) for s in TINY_LEVELS] + [tiny_pyramid_case()]
    cs += [tpw_case(k) for k in ('tpw5', 'tpw2', 'tpw8')]
    cs += [degenerate_case()] + [big_case(K) for K in BIG_K]
    return cs
