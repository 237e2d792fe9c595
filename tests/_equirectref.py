"""numpy float64 restatement of the equirectangular view contract (include/pigeon_hip.h, pg_equirect_*; DESIGN.md "Equirectangular
panoramas in") and the comparator the GPU tests hold the kernel to.  No torch, no library: host arithmetic only.

Per pixel (row i, column j) of an S x S view of an H x W source, IEEE float64, in this order:
    x = (j + 0.5 - S/2) * inv_f                 y = (i + 0.5 - S/2) * inv_f
    w_k = (R[k][0]*x + R[k][1]*y) + R[k][2]
    lam = atan2(w_X, w_Z)                       phi = atan2(-w_Y, sqrt(w_X*w_X + w_Z*w_Z))
    u = (lam*(1/(2 pi)) + 0.5)*W - 0.5          v = (0.5 - phi*(1/pi))*H - 0.5, clamped to [0, H - 1]
    u0 = floor(u), v0 = floor(v), a = floor((u - u0)*256 + 0.5), b = floor((v - v0)*256 + 0.5)
    columns u0 mod W, (u0 + 1) mod W; rows v0, min(v0 + 1, H - 1)
    out = (p00*(256-a)*(256-b) + p01*a*(256-b) + p10*(256-a)*b + p11*a*b + 32768) >> 16

Only atan2 and sqrt can differ between a device's math library and numpy's, by a few ulp: that moves u*256 by about 1e-9 at
W = 16384 and can change a or b by one where the rounded quantity lies that close to an integer.  The comparator therefore
classifies every pixel FROM THE RESTATEMENT ALONE:
    tight  (u - u0)*256 + 0.5 and (v - v0)*256 + 0.5 are each farther than TIE (1e-6, i.e. 4e-9 of a source pixel) from an integer
           -- a v the clamp moved is exact and counts as tight -- and the ray is farther than POLE (1e-9 rad) from a pole;
           such a pixel must be EQUAL, no tolerance;
    loose  everything else: it must equal one of the values the restatement gives for (a + {-1,0,1}, b + {-1,0,1});
    a pixel within POLE of a pole (lam is undefined there) is left out.
A u or v that is an integer within 1e-6 is harmless: (k, 0) and (k - 1, 256) give the same value.
The comparator stays honest while few pixels are loose: `loose_share` of every case of CASES is at most MAX_LOOSE_SHARE (the CPU
test asserts it)."""
import numpy as np

TIE = 1e-6
POLE = 1e-9
MAX_LOOSE_SHARE = 0.01

# (name, source (H, W), view size S, yaw, pitch, fov) -- degrees.  The smallest shapes at which the kernel can still go wrong: a single
# source pixel, a single view pixel (byte tail only), odd widths, S*S mod 4 != 0 (21, 41), more than one block (41*41/4 > 256), the
# seam (yaw 180), both poles (clamped rows), and one large source at the product's view size.
CASES = [
    ("1x1_s1", (1, 1), 1, 0.0, 0.0, 90.0),
    ("1x2_s2", (1, 2), 2, 270.0, 0.0, 90.0),
    ("4x8_s2", (4, 8), 2, 0.0, 0.0, 120.0),
    ("4x8_s21", (4, 8), 21, 90.0, 0.0, 90.0),
    ("17x33_s21", (17, 33), 21, 37.5, -20.0, 75.0),
    ("32x64_s24_seam", (32, 64), 24, 180.0, 0.0, 90.0),
    ("32x64_s24_y90", (32, 64), 24, 90.0, 0.0, 90.0),
    ("32x64_s24_y270_fov120", (32, 64), 24, 270.0, 0.0, 120.0),
    ("64x128_s41_up", (64, 128), 41, 0.0, 90.0, 90.0),
    ("64x128_s41_down", (64, 128), 41, 37.5, -90.0, 90.0),
    ("2048x4096_s336", (2048, 4096), 336, 0.0, 0.0, 90.0),
]


def view_rotation(yaw_deg, pitch_deg):
    """The matrix of the contract, written out: [[C, Sn*s, Sn*c], [0, c, -s], [-Sn, C*s, C*c]]."""
    yw, pt = np.deg2rad(np.float64(yaw_deg)), np.deg2rad(np.float64(pitch_deg))
    C, Sn, c, s = np.cos(yw), np.sin(yw), np.cos(pt), np.sin(pt)
    return np.array([[C, Sn * s, Sn * c], [0.0, c, -s], [-Sn, C * s, C * c]], dtype=np.float64)


def inv_focal(fov_deg, S):
    return float(np.tan(np.deg2rad(np.float64(fov_deg)) / 2) / (np.float64(S) / 2))


def case_params(case):
    """(H, W, S, rot, inv_f) of a CASES entry."""
    _, (H, W), S, yaw, pitch, fov = case
    return H, W, S, view_rotation(yaw, pitch), inv_focal(fov, S)


def rays(S, rot, inv_f):
    """(w_X, w_Z, w_Y) ... returned as (wx, wy, wz), each (S, S) float64."""
    rot = np.asarray(rot, dtype=np.float64).reshape(3, 3)
    half = np.float64(S) / 2
    x = ((np.arange(S, dtype=np.float64) + 0.5 - half) * np.float64(inv_f))[None, :]
    y = ((np.arange(S, dtype=np.float64) + 0.5 - half) * np.float64(inv_f))[:, None]
    return tuple((rot[k, 0] * x + rot[k, 1] * y) + rot[k, 2] for k in range(3))


def angles(S, rot, inv_f):
    """(lam, phi) per pixel."""
    wx, wy, wz = rays(S, rot, inv_f)
    return np.arctan2(wx, wz), np.arctan2(-wy, np.sqrt(wx * wx + wz * wz))


def coords(H, W, S, rot, inv_f):
    """Everything of a view that does not depend on the source's bytes: a dict of (S, S) arrays -- u0, a, v0, b (int64), fa, fb (the
    quantities whose floors a and b are, float64), clamped (v was moved by the clamp) and pole (angle between the ray and the nearer
    pole, radians)."""
    wx, wy, wz = rays(S, rot, inv_f)
    hyp = np.sqrt(wx * wx + wz * wz)
    lam, phi = np.arctan2(wx, wz), np.arctan2(-wy, hyp)
    u = (lam * (1 / (2 * np.pi)) + 0.5) * np.float64(W) - 0.5
    vr = (0.5 - phi * (1 / np.pi)) * np.float64(H) - 0.5
    v = np.minimum(np.maximum(vr, 0.0), np.float64(H - 1))
    u0, v0 = np.floor(u), np.floor(v)
    fa, fb = (u - u0) * 256 + 0.5, (v - v0) * 256 + 0.5
    return dict(u0=u0.astype(np.int64), v0=v0.astype(np.int64), a=np.floor(fa).astype(np.int64), b=np.floor(fb).astype(np.int64),
                fa=fa, fb=fb, clamped=(vr < 0.0) | (vr > np.float64(H - 1)), pole=np.arctan2(hyp, np.abs(wy)))


def blend(src, co, da=0, db=0):
    """The integer half of the contract on `coords`, with a and b moved by (da, db): a step past 0 or 256 carries into u0 / v0 (the
    same position in 1/256ths of a source pixel); a row position pushed off the source stays at its edge.  (0, 0) is the contract."""
    H, W = src.shape[:2]
    u0, v0, a, b = co["u0"].copy(), co["v0"].copy(), co["a"] + da, co["b"] + db
    lo, hi = a < 0, a > 256
    u0[lo] -= 1; a[lo] += 256; u0[hi] += 1; a[hi] -= 256
    lo, hi = b < 0, b > 256
    v0[lo] -= 1; b[lo] += 256; v0[hi] += 1; b[hi] -= 256
    under, over = v0 < 0, v0 > H - 1
    v0[under] = 0; b[under] = 0; v0[over] = H - 1; b[over] = 0
    c0, c1 = np.mod(u0, W), np.mod(u0 + 1, W)
    r0, r1 = v0, np.minimum(v0 + 1, H - 1)
    s = src.astype(np.int64)
    a, b = a[..., None], b[..., None]
    out = (s[r0, c0] * (256 - a) * (256 - b) + s[r0, c1] * a * (256 - b) + s[r1, c0] * (256 - a) * b + s[r1, c1] * a * b + 32768) >> 16
    return out.astype(np.uint8)


def render(src, S, rot, inv_f):
    """The view (S, S, 3) uint8 of the (H, W, 3) uint8 source."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[2] == 3
    return blend(src, coords(src.shape[0], src.shape[1], S, rot, inv_f))


def _far_from_integer(f):
    return np.abs(f - np.round(f)) > TIE


def classify(co):
    """(tight, skipped) boolean (S, S) masks; loose = ~tight & ~skipped."""
    skipped = co["pole"] <= POLE
    tight = _far_from_integer(co["fa"]) & (co["clamped"] | _far_from_integer(co["fb"])) & ~skipped
    return tight, skipped


def loose_share(H, W, S, rot, inv_f):
    """Share of the view's pixels that are not tight (skipped ones included)."""
    tight, _ = classify(coords(H, W, S, rot, inv_f))
    return 1.0 - float(tight.mean())


def compare(got, src, S, rot, inv_f, view=0):
    """AssertionError naming view, row and column of the first pixel of `got` (S, S, 3) the contract does not allow."""
    src, got = np.asarray(src), np.asarray(got)
    assert got.shape == (S, S, 3) and got.dtype == np.uint8, f"view {view}: shape {got.shape} dtype {got.dtype}, expected ({S}, {S}, 3) uint8"
    co = coords(src.shape[0], src.shape[1], S, rot, inv_f)
    want = blend(src, co)
    tight, skipped = classify(co)
    differs = (got != want).any(axis=2) & ~skipped
    bad = differs & tight
    loose = differs & ~tight
    if loose.any():
        ok = np.zeros_like(loose)
        for da in (-1, 0, 1):
            for db in (-1, 0, 1):
                ok |= (got == blend(src, co, da, db)).all(axis=2)
        bad |= loose & ~ok
    if bad.any():
        i, j = (int(t[0]) for t in np.nonzero(bad))
        kind = "tight" if tight[i, j] else "loose"
        raise AssertionError(f"view {view}: row {i}, column {j} ({kind}): got {got[i, j].tolist()}, the contract gives {want[i, j].tolist()} "
                             f"(u0 {int(co['u0'][i, j])}, a {int(co['a'][i, j])}, v0 {int(co['v0'][i, j])}, b {int(co['b'][i, j])}); "
                             f"{int(bad.sum())} of {S * S} pixels wrong")


def random_source(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W, 3), dtype=np.uint8)


def location_source(H, W):
    """R, G, B encode the pixel's own column and row (R: column mod 256, G: row mod 256, B: column // 256 * 16 + row // 256): a wrong
    source pixel shows as a location."""
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.stack([c % 256, r % 256, (c // 256) * 16 + r // 256], axis=2).astype(np.uint8)
