"""Reference for the polar scan format (include/liodom_hip.h, "polar scans"): a NumPy float32 restatement of the projection
arithmetic, the blob layout, designed blobs that hit every special value, and a quantiser that turns a generator scan into a
polar scan.  Pure NumPy: no library, no GPU.  Shared by test_polar_format.py (host) and test_gpu_polar.py (device)."""
import numpy as np

F = np.float32
NAN_BITS = np.uint32(0x7FC00000)


def align16(x):
    return (int(x) + 15) & ~15


def layout(height, width, range_bits, intensity_bits):
    """(tick_offset, range_offset, intensity_offset, total_bytes): every section on a 16-byte boundary, the total a multiple of 16;
    without an intensity section its offset is the total."""
    n = height * width
    r = align16(4 * width)
    i = align16(r + n * range_bits // 8)
    return 0, r, i, align16(i + n * intensity_bits // 8)


class Scan:
    """A geometry (tables as float32 arrays) with one scan's ticks, counts and intensities; order = the handle's lidar_type."""

    def __init__(self, order, height, width, range_bits, intensity_bits, range_unit, beam_origin, cos_alt, sin_alt, cos_baz, sin_baz,
                 cos_enc, sin_enc, ticks, counts, intensities):
        self.order, self.height, self.width = order, height, width
        self.range_bits, self.intensity_bits = range_bits, intensity_bits
        self.range_unit, self.beam_origin = F(range_unit), F(beam_origin)
        self.cos_alt, self.sin_alt, self.cos_baz, self.sin_baz = (np.asarray(a, F) for a in (cos_alt, sin_alt, cos_baz, sin_baz))
        self.cos_enc, self.sin_enc = np.asarray(cos_enc, F), np.asarray(sin_enc, F)
        self.ticks = np.asarray(ticks, np.uint32)
        self.counts = np.asarray(counts, np.uint16 if range_bits == 16 else np.uint32)
        self.intensities = None if intensity_bits == 0 else np.asarray(intensities, np.uint8 if intensity_bits == 8 else np.uint16)
        assert self.cos_alt.shape == (height,) and self.ticks.shape == (width,) and self.counts.shape == (height * width,)

    @property
    def T(self):
        return int(self.cos_enc.shape[0])

    def blob(self):
        _, r, i, total = layout(self.height, self.width, self.range_bits, self.intensity_bits)
        b = np.zeros(total, np.uint8)
        for off, a in ((0, self.ticks), (r, self.counts), (i, self.intensities)):
            if a is not None:
                raw = a.astype(a.dtype.newbyteorder("<")).view(np.uint8)
                b[off:off + raw.size] = raw
        return b


def project(s):
    """The packed cloud [H W, 4] of a Scan: element-wise float32 products and sums, each rounded on its own, in the order the
    header gives.  Invalid points (count 0, tick >= T) get the quiet NaN 0x7FC00000 in x y z and keep w."""
    n = s.height * s.width
    i = np.arange(n)
    row, col = (i % s.height, i // s.height) if s.order == 0 else (i // s.width, i % s.width)
    t = s.ticks[col].astype(np.int64)
    ok = t < s.T
    ts = np.where(ok, t, 0)                  # (never index with a tick that failed the test)
    ce, se = s.cos_enc[ts], s.sin_enc[ts]
    ca, sa, cb, sb = s.cos_alt[row], s.sin_alt[row], s.cos_baz[row], s.sin_baz[row]
    r = s.counts.astype(np.uint32).astype(F) * s.range_unit
    d = r - s.beam_origin
    h = d * ca
    ct = ce * cb - se * sb
    st = se * cb + ce * sb
    out = np.zeros((n, 4), F)
    out[:, 0] = h * ct + s.beam_origin * ce
    out[:, 1] = h * st + s.beam_origin * se
    out[:, 2] = d * sa
    out[:, 3] = 0 if s.intensities is None else s.intensities.astype(F)
    assert out.dtype == F and r.dtype == F and ct.dtype == F
    bad = (s.counts == 0) | ~ok
    out.view(np.uint32)[bad, :3] = NAN_BITS
    return out


# ---- designed blobs -----------------------------------------------------------------------------------------------------------
# (name, order, H, W, range_bits, intensity_bits, T, beam origin and beam azimuth non-zero)
DESIGNED = [
    ("t0_16x70_r16_i8", 0, 16, 70, 16, 8, 70, False),
    ("t0_16x70_r32_i16_bigT", 0, 16, 70, 32, 16, 90112, True),
    ("t0_16x33_r32_i0_T1", 0, 16, 33, 32, 0, 1, True),
    ("t1_5x131_r16_i0_T1", 1, 5, 131, 16, 0, 1, True),
    ("t1_5x131_r32_i8", 1, 5, 131, 32, 8, 131, False),
    ("t1_128x33_r32_i8_bigT", 1, 128, 33, 32, 8, 90112, False),
    ("t1_128x33_r16_i16", 1, 128, 33, 16, 16, 2048, True),
    ("t1_1x1_r16_i16_T1", 1, 1, 1, 16, 16, 1, True),
    ("t1_1x1_r32_i8", 1, 1, 1, 32, 8, 7, False),
]


def designed(name):
    """The Scan of a DESIGNED row: random tables, counts, intensities and non-monotone ticks, with the special values put in:
    counts 0, 1 and the width's maximum (32-bit: also 2^24 + 1, which rounds); intensity 0 and its maximum; ticks 0, T - 1, T and
    0xFFFFFFFF (the last two make NaN columns).  Specials land on distinct points of valid columns where the shape has room."""
    _, order, H, W, rb, ib, T, nz = next(r for r in DESIGNED if r[0] == name)
    rng = np.random.default_rng(sum(map(ord, name)) * 7919)
    n = H * W
    alt = rng.uniform(-0.45, 0.3, H)
    baz = rng.uniform(-0.06, 0.06, H) if nz else np.zeros(H)
    enc = rng.uniform(-np.pi, np.pi, T)
    cmax = (1 << rb) - 1
    counts = rng.integers(1, min(cmax, 60000) + 1, n, dtype=np.uint64)
    special_ticks = [0, T - 1, T, 0xFFFFFFFF]
    ticks = rng.integers(0, T, W, dtype=np.uint64)
    for k, v in enumerate(special_ticks[:W] if W >= 4 else special_ticks[1:1 + W]):
        ticks[k] = v
    # points of a column with a valid tick, spread over rows, for the special counts and intensities
    i = np.arange(n)
    col = (i // H) if order == 0 else (i % W)
    valid = np.flatnonzero(ticks[col] < T)
    special_counts = [0, 1, cmax] + ([(1 << 24) + 1] if rb == 32 else [])
    for k, v in enumerate(special_counts):         # (a 1 x 1 scan keeps the last one)
        counts[valid[(k * 37) % valid.size]] = v
    inten = None
    if ib:
        imax = (1 << ib) - 1
        inten = rng.integers(0, imax + 1, n, dtype=np.uint64)
        inten[0] = imax
        inten[-1 if n > 1 else 0] = 0 if n > 1 else imax
        if n > 2:
            inten[n // 2] = 0
    return Scan(order, H, W, rb, ib, 0.002 if rb == 16 else 0.001, 0.015806 if nz else 0.0, np.cos(alt), np.sin(alt), np.cos(baz), np.sin(baz),
                np.cos(enc), np.sin(enc), ticks, counts, inten)


# ---- quantiser: a generator scan as a polar scan ---------------------------------------------------------------------------------
def quantise(xyzi, height, width, order, range_bits=16, intensity_bits=8, tables=None):
    """A Scan for a packed cloud of the synthetic generator: altitude of a row = the median elevation of its returns, azimuth of a
    column = the direction of the sum of its returns' horizontal unit vectors, tick = column with T = W, 2 mm per count, NaN and
    zero-range returns become count 0; no beam origin, no beam azimuth.  tables: (cos_alt, sin_alt, cos_enc, sin_enc) of an
    earlier scan of the same stream to reuse — a geometry is set once per handle."""
    x = np.asarray(xyzi, np.float64).reshape(-1, 4)
    n = height * width
    i = np.arange(n)
    row, col = (i % height, i // height) if order == 0 else (i // width, i % width)
    rng = np.sqrt((x[:, :3] ** 2).sum(1))
    good = np.isfinite(rng) & (rng > 0)
    if tables is None:
        hor = np.sqrt(x[:, 0] ** 2 + x[:, 1] ** 2)
        with np.errstate(invalid="ignore", divide="ignore"):
            el = np.arctan2(x[:, 2], hor)
            ux, uy = x[:, 0] / hor, x[:, 1] / hor
        alt = np.array([np.median(el[good & (row == r)]) if (good & (row == r)).any() else 0.0 for r in range(height)])
        g2 = good & (hor > 0)
        sx = np.bincount(col[g2], ux[g2], width)
        sy = np.bincount(col[g2], uy[g2], width)
        az = np.where((sx == 0) & (sy == 0), 2 * np.pi * np.arange(width) / width, np.arctan2(sy, sx))
        tables = (np.cos(alt), np.sin(alt), np.cos(az), np.sin(az))
    unit = 0.002
    counts = np.where(good, np.minimum(np.rint(np.where(good, rng, 0) / unit), (1 << range_bits) - 1), 0).astype(np.uint64)
    inten = None if intensity_bits == 0 else ((row * 37 + col) & ((1 << intensity_bits) - 1))
    return Scan(order, height, width, range_bits, intensity_bits, unit, 0.0, tables[0], tables[1], np.ones(height), np.zeros(height),
                tables[2], tables[3], np.arange(width), counts, inten)
