"""The synthetic generator's rolling sweep (synth make_cfg(sweep=1)) and the deskew model of tests/deskewref.py: the input on which
deskewing by the predicted scan motion was measured ("Finding: deskewing by the predicted motion does not pay on the
synthetic sweep").  CPU only."""
import math

import numpy as np
import pytest

import deskewref as dr

SHAPES = [(16, 1800, 0), (32, 512, 1)]   # VLP-16 firing order, Ouster row-major


def _rodrigues(axis, phi):
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    return np.eye(3) + math.sin(phi) * K + (1.0 - math.cos(phi)) * (K @ K)


def _columns(x, H, W, lt):
    idx = np.arange(H * W)
    return (idx // H) if lt == 0 else (idx % W)


@pytest.mark.parametrize("H,W,lt", SHAPES)
def test_sweep_off_is_the_default_stream(synth, H, W, lt):
    base = synth.make_cfg(H, W, lt, speed=1.0, yaw_rate_deg=3.0)
    off = synth.make_cfg(H, W, lt, speed=1.0, yaw_rate_deg=3.0, sweep=0)
    on = synth.make_cfg(H, W, lt, speed=1.0, yaw_rate_deg=3.0, sweep=1)
    for k in (0, 5):
        x0, g0 = synth.scan(base, 0, k)
        x1, g1 = synth.scan(off, 0, k)
        x2, g2 = synth.scan(on, 0, k)
        assert np.array_equal(x0.view(np.uint32), x1.view(np.uint32))
        assert np.array_equal(g0, g1) and np.array_equal(g0, g2), "the ground truth is the pose at the end of the sweep"
        assert not np.array_equal(x0.view(np.uint32), x2.view(np.uint32)), "sweep=1 must move the columns"


@pytest.mark.parametrize("H,W,lt", SHAPES)
def test_sweep_columns_give_their_sweep_fraction(synth, H, W, lt):
    cfg = synth.make_cfg(H, W, lt, speed=1.0, yaw_rate_deg=3.0, sweep=1)
    x, _ = synth.scan(cfg, 0, 7)
    c = _columns(x, H, W, lt)
    ok = np.isfinite(x[:, 0])
    assert ok.sum() > H * W // 4
    s = dr.sweep_fraction(x[ok, :3], 1, 0.0)
    err = np.abs((s - c[ok] / W + 0.5) % 1.0 - 0.5)
    assert err.max() < 1e-5, err.max()
    s_cw = dr.sweep_fraction(x[ok, :3], -1, 0.0)          # the other spin direction reverses the sweep
    assert np.abs((s_cw + s + 0.5) % 1.0 - 0.5).max() < 1e-5


@pytest.mark.parametrize("H,W,lt", SHAPES)
def test_sweep_distortion_follows_the_model(synth, H, W, lt):
    """Every column is cast from T_{k-1} D^{s_c}: expressed in the end-of-sweep frame its points are R(u theta)^T (p - u t) away
    from where the sensor put them; deskewing with the generator's own motion puts them back, up to the model's second-order
    term u (1 - u) theta |t| (1.3 cm at 1 m and 3 degrees per scan)."""
    cfg = synth.make_cfg(H, W, lt, speed=1.0, yaw_rate_deg=3.0, sweep=1, noise_sigma=0.0)
    k = 9
    x, g = synth.scan(cfg, 0, k)
    _, g_prev = synth.scan(cfg, 0, k - 1)
    T, T0 = dr.pose34(g), dr.pose34(g_prev)
    D = dr.delta_of(T0, T)
    axis, theta, t = dr.motion(D)
    assert abs(math.degrees(theta) - 3.0) < 0.05 and abs(np.linalg.norm(t) - 1.0) < 0.01
    ok = np.isfinite(x[:, 0])
    pts, cols = x[ok], _columns(x, H, W, lt)[ok]
    want = np.zeros((pts.shape[0], 3))
    for c in np.unique(cols):
        s = c / W
        Rc = T0[:, :3] @ _rodrigues(axis, s * theta)
        tc = T0[:, 3] + s * (T0[:, :3] @ t)
        m = cols == c
        world = pts[m, :3].astype(np.float64) @ Rc.T + tc
        want[m] = (world - T[:, 3]) @ T[:, :3]          # into the end-of-sweep frame
    raw_err = np.linalg.norm(pts[:, :3] - want, axis=1)
    fixed = dr.deskew_edges(pts, D, 1, 0.0)
    fixed_err = np.linalg.norm(fixed[:, :3] - want, axis=1)
    assert raw_err.mean() > 0.3, raw_err.mean()
    assert fixed_err.max() < 0.02, fixed_err.max()
    assert np.array_equal(fixed[:, 3], pts[:, 3]), "intensity is unchanged"


def test_deskew_reference_identity_is_bit_exact(synth):
    x, _ = synth.scan(synth.make_cfg(16, 900, 0, sweep=1), 0, 3)
    e = x[np.isfinite(x[:, 0])]
    e[:3, 0] = -0.0
    I = np.hstack([np.eye(3), np.zeros((3, 1))])
    I_neg = I.copy()
    I_neg[:, 3] = -0.0
    for D in (I, I_neg):
        for direction in (1, -1):
            out = dr.deskew_edges(e, D, direction, 37.0)
            assert np.array_equal(out.view(np.uint32), e.view(np.uint32))
