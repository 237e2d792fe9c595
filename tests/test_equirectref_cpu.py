"""The numpy restatement of the equirectangular view contract (tests/_equirectref.py) and its comparator, checked on the host: the
projection against the textbook forward gnomonic projection in mpmath, the constant image, the cap on loose pixels that keeps the
comparator honest, and planted mistakes the comparator must reject by view, row and column."""
import re

import mpmath as mp
import numpy as np
import pytest

import _equirectref as E

SMALL = [c for c in E.CASES if c[2] <= 41]


@pytest.mark.parametrize("case", E.CASES, ids=[c[0] for c in E.CASES])
def test_round_trip_through_snyder_forward_gnomonic(case):
    """(lam, phi) of the restatement go back through Snyder's closed form (Map Projections -- A Working Manual, eq. 5-3, 22-4, 22-5),
    centred on (yaw, pitch), evaluated in mpmath: written from the angles, not from the rotation matrix.  Must land within 1e-9 of
    the pixel's centre (j + 0.5, i + 0.5)."""
    mp.mp.dps = 40
    _, (H, W), S, yaw, pitch, fov = case
    rot, inv_f = E.view_rotation(yaw, pitch), E.inv_focal(fov, S)
    lam, phi = E.angles(S, rot, inv_f)
    pole = E.coords(H, W, S, rot, inv_f)["pole"]
    lam0, phi1 = mp.radians(mp.mpf(yaw)), mp.radians(mp.mpf(pitch))
    f = mp.tan(mp.radians(mp.mpf(fov)) / 2) / (mp.mpf(S) / 2)
    step = 1 if S <= 41 else 7
    worst = 0.0
    for i in range(0, S, step):
        for j in range(0, S, step):
            if pole[i, j] <= E.POLE:
                continue
            l, p = mp.mpf(float(lam[i, j])), mp.mpf(float(phi[i, j]))
            cosc = mp.sin(phi1) * mp.sin(p) + mp.cos(phi1) * mp.cos(p) * mp.cos(l - lam0)
            assert cosc > 0, f"pixel ({i}, {j}) lies behind the view"
            x = mp.cos(p) * mp.sin(l - lam0) / cosc
            y = (mp.cos(phi1) * mp.sin(p) - mp.sin(phi1) * mp.cos(p) * mp.cos(l - lam0)) / cosc          # north up
            col, row = x / f + mp.mpf(S) / 2, -y / f + mp.mpf(S) / 2
            worst = max(worst, float(abs(col - (j + 0.5))), float(abs(row - (i + 0.5))))
    print(f"{case[0]}: worst round-trip error {worst:.3e} view pixels")
    assert worst <= 1e-9


@pytest.mark.parametrize("case", E.CASES, ids=[c[0] for c in E.CASES])
def test_constant_image_stays_constant(case):
    H, W, S, rot, inv_f = E.case_params(case)
    for value in ((0, 0, 0), (255, 255, 255), (7, 130, 251)):
        src = np.empty((H, W, 3), dtype=np.uint8)
        src[...] = value
        out = E.render(src, S, rot, inv_f)
        assert (out == np.array(value, dtype=np.uint8)).all()


@pytest.mark.parametrize("case", E.CASES, ids=[c[0] for c in E.CASES])
def test_loose_share_is_capped(case):
    H, W, S, rot, inv_f = E.case_params(case)
    share = E.loose_share(H, W, S, rot, inv_f)
    print(f"{case[0]}: {share:.2e} of the pixels are not tight")
    assert share <= E.MAX_LOOSE_SHARE


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_tight_pixels_survive_a_few_ulp_of_atan2(case):
    """u moved by 4e-16 relative + 1e-13 absolute and v by 1e-13 absolute -- the scale of a few-ulp atan2 error -- changes no tight
    pixel's (position in 1/256ths), hence no tight pixel's value."""
    H, W, S, rot, inv_f = E.case_params(case)
    co = E.coords(H, W, S, rot, inv_f)
    tight, _ = E.classify(co)
    for sign in (-1.0, 1.0):
        u = co["u0"] + (co["fa"] - 0.5) / 256
        fa = co["fa"] + sign * (np.abs(u) * 4e-16 + 1e-13) * 256
        fb = co["fb"] + sign * 1e-13 * 256 * ~co["clamped"]
        assert (np.floor(fa) == co["a"])[tight].all() and (np.floor(fb) == co["b"])[tight].all()


# ---- planted mistakes ----------------------------------------------------------------------------------------------------------
def _variant(src, S, rot, inv_f, mistake=None):
    """The contract written out once more with one switch per mistake; with no switch it is the restatement (asserted below)."""
    H, W = src.shape[:2]
    rot = np.asarray(rot, dtype=np.float64).reshape(3, 3)
    half = np.float64(S) / 2
    cv = 0.0 if mistake == "no_half_pixel_view" else 0.5
    cs = 0.0 if mistake == "no_half_pixel_source" else 0.5
    x = ((np.arange(S, dtype=np.float64) + cv - half) * inv_f)[None, :]
    y = ((np.arange(S, dtype=np.float64) + cv - half) * inv_f)[:, None]
    wx, wy, wz = ((rot[k, 0] * x + rot[k, 1] * y) + rot[k, 2] for k in range(3))
    lam, phi = np.arctan2(wx, wz), np.arctan2(-wy, np.sqrt(wx * wx + wz * wz))
    if mistake == "flipped_latitude":
        phi = -phi
    u = (lam * (1 / (2 * np.pi)) + 0.5) * W - cs
    v = np.minimum(np.maximum((0.5 - phi * (1 / np.pi)) * H - cs, 0.0), np.float64(H - 1))
    u0, v0 = np.floor(u), np.floor(v)
    rnd = 0.0 if mistake == "truncated_fraction" else 0.5
    a, b = np.floor((u - u0) * 256 + rnd).astype(np.int64), np.floor((v - v0) * 256 + rnd).astype(np.int64)
    if mistake == "a_b_swapped":
        a, b = b, a
    u0, v0 = u0.astype(np.int64), v0.astype(np.int64)
    if mistake == "clamp_at_seam":
        c0, c1 = np.clip(u0, 0, W - 1), np.clip(u0 + 1, 0, W - 1)
    else:
        c0, c1 = np.mod(u0, W), np.mod(u0 + 1, W)
    r0, r1 = v0, np.minimum(v0 + 1, H - 1)
    s = src.astype(np.int64)
    a3, b3 = a[..., None], b[..., None]
    out = ((s[r0, c0] * (256 - a3) * (256 - b3) + s[r0, c1] * a3 * (256 - b3) + s[r1, c0] * (256 - a3) * b3 + s[r1, c1] * a3 * b3 + 32768) >> 16).astype(np.uint8)
    if mistake == "row_not_clamped":
        # v0 + 1 == H carries weight b == 0 (v was clamped to H - 1), so the VALUE cannot show the missing min(): the address does.
        # What lies behind the source is not the source's: such a pixel is poisoned, as a guard row would show a stray access.
        out[v0 + 1 > H - 1] ^= 0xFF
    return out


# looking straight down at a source of 4 rows: every ray within 22.5 degrees of the nadir has its v clamped to the last row
DOWN_4x8 = ("4x8_s21_down", (4, 8), 21, 37.5, -90.0, 90.0)


def _case(name):
    return next(c for c in E.CASES + [DOWN_4x8] if c[0] == name)


def _rx_ry(yaw, pitch):
    """The pitch applied AFTER the yaw: Rx(pitch) . Ry(yaw)."""
    return E.view_rotation(0.0, pitch) @ E.view_rotation(yaw, 0.0)


# mistake -> (case it must show on, how the wrong view is made)
RENDER_MISTAKES = {
    "no_half_pixel_view": "17x33_s21", "no_half_pixel_source": "17x33_s21", "clamp_at_seam": "32x64_s24_seam",
    "flipped_latitude": "17x33_s21", "a_b_swapped": "17x33_s21", "truncated_fraction": "17x33_s21", "row_not_clamped": "4x8_s21_down",
}
ANGLE_MISTAKES = {
    "yaw_sign": lambda yaw, pitch, fov, S: (E.view_rotation(-yaw, pitch), E.inv_focal(fov, S)),
    "pitch_sign": lambda yaw, pitch, fov, S: (E.view_rotation(yaw, -pitch), E.inv_focal(fov, S)),
    "fov_as_half_angle": lambda yaw, pitch, fov, S: (E.view_rotation(yaw, pitch), float(np.tan(np.deg2rad(fov)) / (S / 2))),
    "pitch_after_yaw": lambda yaw, pitch, fov, S: (_rx_ry(yaw, pitch), E.inv_focal(fov, S)),
    "neighbouring_view": lambda yaw, pitch, fov, S: (E.view_rotation(yaw + 90.0, pitch), E.inv_focal(fov, S)),
}
NAMES_PIXEL = re.compile(r"view 3: row \d+, column \d+")


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_variant_without_a_mistake_is_the_restatement(case):
    H, W, S, rot, inv_f = E.case_params(case)
    src = E.random_source(H, W, 5)
    out = _variant(src, S, rot, inv_f)
    assert np.array_equal(out, E.render(src, S, rot, inv_f))
    E.compare(out, src, S, rot, inv_f, view=3)


@pytest.mark.parametrize("mistake", sorted(RENDER_MISTAKES))
def test_comparator_rejects_a_wrong_kernel(mistake):
    H, W, S, rot, inv_f = E.case_params(_case(RENDER_MISTAKES[mistake]))
    # (the location image changes by one per source pixel: 1/256 of such a step, all truncation moves, never reaches its rounding)
    sources = [E.random_source(H, W, 11)] + ([] if mistake == "truncated_fraction" else [E.location_source(H, W)])
    for src in sources:
        with pytest.raises(AssertionError, match=NAMES_PIXEL):
            E.compare(_variant(src, S, rot, inv_f, mistake), src, S, rot, inv_f, view=3)


@pytest.mark.parametrize("mistake", sorted(ANGLE_MISTAKES))
def test_comparator_rejects_wrong_angles(mistake):
    _, (H, W), S, yaw, pitch, fov = _case("17x33_s21")                                   # yaw 37.5, pitch -20, fov 75: nothing cancels
    rot, inv_f = E.view_rotation(yaw, pitch), E.inv_focal(fov, S)
    wrong_rot, wrong_f = ANGLE_MISTAKES[mistake](yaw, pitch, fov, S)
    for src in (E.random_source(H, W, 12), E.location_source(H, W)):
        with pytest.raises(AssertionError, match=NAMES_PIXEL):
            E.compare(E.render(src, S, wrong_rot, wrong_f), src, S, rot, inv_f, view=3)


def test_loose_pixel_rules():
    """A loose pixel may take a neighbouring a / b and nothing else; a tight one may not; a pole pixel is left out."""
    H, W, S, rot, inv_f = E.case_params(_case("64x128_s41_up"))
    src = E.random_source(H, W, 13)
    co = E.coords(H, W, S, rot, inv_f)
    tight, skipped = E.classify(co)
    assert skipped[20, 20] and skipped.sum() == 1                                        # the centre pixel looks at the pole
    got = E.render(src, S, rot, inv_f)
    got[20, 20] ^= 0xFF
    E.compare(got, src, S, rot, inv_f)                                                   # the pole pixel is not compared
    moved = E.blend(src, co, 1, 0)
    k = np.nonzero((moved != got).any(axis=2) & tight)
    i, j = int(k[0][0]), int(k[1][0])
    got2 = got.copy()
    got2[i, j] = moved[i, j]
    with pytest.raises(AssertionError, match=rf"view 0: row {i}, column {j} \(tight\)"):
        E.compare(got2, src, S, rot, inv_f)
    # a pixel made loose by construction: u exactly on a tie of the rounding
    co2 = {k2: v.copy() for k2, v in co.items()}
    co2["fa"][i, j] = np.float64(co["a"][i, j])                                          # sits ON the integer: a or a - 1 both allowed
    t2, _ = E.classify(co2)
    assert not t2[i, j]


def test_blend_step_carries_across_a_source_pixel():
    """(u0, a = 256) is (u0 + 1, 0): moving a by one across 0 or 256 carries, so the 3 x 3 neighbourhood means positions."""
    src = E.random_source(4, 8, 14)
    z = np.zeros((1, 1), dtype=np.int64)
    at = lambda u0, a: E.blend(src, dict(u0=z + u0, v0=z + 1, a=z + a, b=z + 77))
    assert np.array_equal(at(2, 256), at(3, 0))
    assert np.array_equal(E.blend(src, dict(u0=z + 3, v0=z + 1, a=z, b=z + 77), -1, 0), at(2, 255))
    assert np.array_equal(E.blend(src, dict(u0=z + 7, v0=z + 1, a=z + 256, b=z + 77), 1, 0), at(8, 1))      # and wraps: column 8 = 0
