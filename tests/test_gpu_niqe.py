"""NIQE on the device (csrc/iqa.hip through the C-ABI) against the float64 oracle tests/niqe_ref.py.

Tolerances are measured, not chosen: the oracle run in float32 (the device's arithmetic for pixels and block sums) against the oracle
in float64 on the very inputs below, times 8 for the device's different summation order over a 9,216-element block.
`python tests/test_gpu_niqe.py` prints the measurements (CPU only). As measured:

    features   max |float32 - float64| = 4.84e-08  ->  FEAT_ATOL  = 3.88e-07   (must stay below 1e-4; E[y^2] - mu^2 in float32: 1.1e-03)
    sharpness  max relative            = 9.62e-08  ->  SHARP_RTOL = 7.70e-07
    score      max relative            = 8.16e-08  ->  SCORE_RTOL = 6.52e-07
    fit        max |mu|, |cov| diff    = 8.86e-09, 2.90e-09  ->  FIT_MU_ATOL = 7.09e-08, FIT_COV_ATOL = 2.32e-08
    shape      float32 and float64 pick a different grid point in 0 of 180 (block, map) fits (bound: 5 %, one step apart)

Gray uint8 inputs make the luma exact, so the feature tests are not disturbed by +-1-level rounding ties; the luma has its own
bit-exact test on RGB inputs.
"""
import os

import numpy as np
import pytest

import niqe_ref as R

FEAT_ATOL = 3.88e-07
SHARP_RTOL = 7.70e-07
SCORE_RTOL = 6.52e-07
FIT_MU_ATOL = 7.09e-08
FIT_COV_ATOL = 2.32e-08
ALPHA_STEP = 0.001
ALPHA_COLS = [0, 2, 6, 10, 14, 18, 20, 24, 28, 32]
REAL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "real")
DET = ("det_family", "det_parade", "det_photo4k", "det_test1")


def _gray(name):
    from PIL import Image
    with Image.open(os.path.join(REAL, name + ".png")) as im:
        return np.ascontiguousarray(np.asarray(im.convert("L")))


def _rgb(name):
    from PIL import Image
    with Image.open(os.path.join(REAL, name + ".png")) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB")))


def _smooth_noise(h, w, seed):
    from scipy.ndimage import gaussian_filter
    a = gaussian_filter(np.random.default_rng(seed).standard_normal((h, w)), 1.5)
    a = (a - a.min()) / (a.max() - a.min())
    return np.ascontiguousarray(np.rint(a * 255).astype(np.uint8))


def cases():
    fam = _gray("det_family")
    return {
        "min_192x96": np.ascontiguousarray(_gray("det_parade")[32:224, 80:176]),      # the two-block minimum
        "crop_200x300": np.ascontiguousarray(fam[12:212, 10:310]),                    # crops to 192 x 288: 6 blocks
        "family_224x320": fam,
        "smooth_noise_210x200": _smooth_noise(210, 200, 7),
    }


def pristine_model(feats, seed=11):
    """A full-rank pristine model near the features: a seeded SPD matrix with condition number 1e3, scaled by the features' spread."""
    rng = np.random.default_rng(seed)
    sd = np.nanstd(feats, axis=0) + 1e-3
    q, _ = np.linalg.qr(rng.standard_normal((36, 36)))
    cov = (q * np.logspace(0, -3, 36)) @ q.T
    cov = (cov + cov.T) / 2 * np.outer(sd, sd)
    return np.nanmean(feats, axis=0) + 0.5 * sd * rng.standard_normal(36), cov


def nan_image():
    """192 x 192, the first block flat: the constant reaches 16 pixels past the block, further than the half-size taps (4 pixels) plus
    the scale-2 window (3 pixels at half size) look."""
    img = _smooth_noise(192, 192, 5)
    img[:112, :112] = 90
    return img


@pytest.fixture(scope="module")
def ref():
    out = {k: R.features(v) for k, v in cases().items()}
    out["nan"] = R.features(nan_image())
    return out


@pytest.fixture(scope="module")
def iqa(gpu_lib):
    q = gpu_lib.IQA(0)
    yield q
    q.close()


def _check_features(got, sharp, img, want, want_sharp):
    """The issue's comparison: shapes equal or one grid step apart; everything else against the oracle at the device's shapes."""
    ga, wa = got[:, ALPHA_COLS].astype(np.float64), want[:, ALPHA_COLS]
    steps = np.rint((ga - wa) / ALPHA_STEP)
    assert np.all(np.abs(ga - (wa + steps * ALPHA_STEP)) < 1e-6) and np.all(np.abs(steps) <= 1), (ga, wa)
    at = want if not steps.any() else R.features(img, alpha=np.rint((ga - 0.2) / ALPHA_STEP) * ALPHA_STEP + 0.2)[0]
    rest = [c for c in range(36) if c not in ALPHA_COLS]
    assert np.array_equal(np.isnan(got), np.isnan(at))
    err = np.nanmax(np.abs(got[:, rest] - at[:, rest]))
    srel = np.max(np.abs(sharp - want_sharp) / want_sharp)
    print(f"features: max |device - oracle| = {err:.3g} (bound {FEAT_ATOL:.3g}); sharpness rel {srel:.3g} (bound {SHARP_RTOL:.3g}); "
          f"{int(np.count_nonzero(steps))} of {steps.size} shapes one step apart")
    assert err <= FEAT_ATOL
    assert srel <= SHARP_RTOL
    return int(np.count_nonzero(steps)), steps.size


@pytest.mark.gpu
def test_features_match_the_float64_oracle(iqa, ref):
    apart = total = 0
    for name, img in cases().items():
        feat, sharp, off = iqa.niqe_features([img])
        want, want_sharp = ref[name]
        assert feat.shape == want.shape and off.tolist() == [0, want.shape[0]] and feat.dtype == np.float64
        a, t = _check_features(feat, sharp, img, want, want_sharp)
        apart, total = apart + a, total + t
    assert apart <= 0.05 * total, (apart, total)


@pytest.mark.gpu
def test_luma_is_the_float32_restatement_bit_for_bit(iqa, gpu_lib):
    rng = np.random.default_rng(2)
    u8 = rng.integers(0, 256, (100, 197, 3), dtype=np.uint8)
    f32 = rng.random((3, 100, 197), dtype=np.float32)
    f32[:, :4, :4] = np.float32([0, 1, 0.5, 1 / 255]).reshape(1, 1, 4)
    for img in (u8, f32, f32[:1], u8[:, :, 0].copy(), _rgb("det_family")):
        got = iqa.luma(img)
        want = R.crop(R.luma(img))
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(iqa.luma(u8[:, :, ::-1].copy(), gpu_lib.CHAN_AS_BGR), R.crop(R.luma(u8)))
    as_float = np.ascontiguousarray(np.moveaxis(u8.astype(np.float32) / np.float32(255), 2, 0))
    a, sa, _ = iqa.niqe_features([u8])
    b, sb, _ = iqa.niqe_features([as_float])
    c, _, _ = iqa.niqe_features([u8[:, :, ::-1].copy()], gpu_lib.CHAN_AS_BGR)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and np.array_equal(sa, sb) and np.array_equal(a.view(np.uint64), c.view(np.uint64))


@pytest.mark.gpu
def test_pixels_outside_the_crop_are_never_read(iqa):
    a = _smooth_noise(100, 200, 3)
    b = a.copy()
    b[96:, :] = 255 - b[96:, :]
    b[:, 192:] = 255 - b[:, 192:]
    assert not np.array_equal(a, b) and np.array_equal(a[:96, :192], b[:96, :192])
    fa, sa, _ = iqa.niqe_features([a])
    fb, sb, _ = iqa.niqe_features([b])
    assert fa.shape == (2, 36) and np.array_equal(fa.view(np.uint64), fb.view(np.uint64)) and np.array_equal(sa, sb)
    want = R.features(a[:96, :192])[0]                   # and the crop's edge is a replicate border
    assert np.nanmax(np.abs(fa[:, [c for c in range(36) if c not in ALPHA_COLS]] - want[:, [c for c in range(36) if c not in ALPHA_COLS]])) <= FEAT_ATOL


@pytest.mark.gpu
def test_an_image_does_not_depend_on_its_batch_mates(iqa, ref):
    cs = cases()
    img = cs["crop_200x300"]
    mu, cov = pristine_model(ref["crop_200x300"][0])
    alone, s_alone, _ = iqa.niqe_features([img])
    batch = [cs["min_192x96"], img, cs["smooth_noise_210x200"]]
    feat, sharp, off = iqa.niqe_features(batch)
    assert off.tolist() == [0, 2, 8, 12]
    assert np.array_equal(feat[2:8].view(np.uint64), alone.view(np.uint64)) and np.array_equal(sharp[2:8], s_alone)
    assert iqa.niqe(batch, mu, cov)[1] == iqa.niqe([img], mu, cov)[0]


@pytest.mark.gpu
def test_flat_block_is_nan_and_the_score_stays_finite(iqa, gpu_lib, ref):
    img = nan_image()
    want, want_sharp = ref["nan"]
    feat, sharp, off = iqa.niqe_features([img])
    assert np.isnan(want[0, 1]) and not np.isnan(want[1:]).any() and want[0, 0] == 0.2
    assert np.array_equal(np.isnan(feat), np.isnan(want))
    assert sharp[0] == 0 and want_sharp[0] == 0
    mu, cov = pristine_model(ref["family_224x320"][0])
    got = gpu_lib.niqe_score(feat, off, mu, cov)[0]
    exp = R.score(want, mu, cov)
    print(f"score with a NaN block: device {got:.9g}, oracle {exp:.9g}, rel {abs(got - exp) / exp:.3g} (bound {SCORE_RTOL:.3g})")
    assert np.isfinite(got) and abs(got - exp) <= SCORE_RTOL * exp


@pytest.mark.gpu
def test_score_matches_the_oracle(iqa, ref):
    cs = cases()
    mu, cov = pristine_model(np.concatenate([ref[k][0] for k in cs]))
    got = iqa.niqe(list(cs.values()), mu, cov)
    for g, k in zip(got, cs):
        exp = R.score(ref[k][0], mu, cov)
        print(f"score {k}: device {g:.9g}, oracle {exp:.9g}, rel {abs(g - exp) / exp:.3g} (bound {SCORE_RTOL:.3g})")
        assert abs(g - exp) <= SCORE_RTOL * exp


@pytest.mark.gpu
def test_too_small_image_is_an_argument_error(iqa, gpu_lib):
    for shape in ((96, 191), (95, 1000), (191, 96)):
        with pytest.raises(gpu_lib.FfpError) as e:
            iqa.niqe_features([np.zeros(shape, np.uint8)])
        assert e.value.code == 1 and "two 96x96 blocks" in str(e.value)
    with pytest.raises(gpu_lib.FfpError):
        iqa.niqe_features([np.zeros((192, 192, 2), np.uint8)])


@pytest.mark.gpu
def test_fit_and_the_pyiqa_shim(iqa, gpu_lib, tmp_path):
    import torch
    import ffp_amd.compat as compat
    from ffp_amd import iqa as iqa_mod
    imgs = [_gray(n) for n in DET]
    mu, cov = iqa_mod.fit_niqe_model(imgs, engine=iqa)
    feat, _, off = iqa.niqe_features(imgs)
    oracle = []
    for i, img in enumerate(imgs):                       # the oracle at the device's shapes (they are checked in the feature test)
        a = np.rint((feat[off[i]:off[i + 1], ALPHA_COLS].astype(np.float64) - 0.2) / ALPHA_STEP) * ALPHA_STEP + 0.2
        oracle.append(R.features(img, alpha=a))
    emu, ecov = R.fit(oracle)
    print(f"fit: max |mu - oracle| = {np.max(np.abs(mu - emu)):.3g} (bound {FIT_MU_ATOL:.3g}), max |cov - oracle| = {np.max(np.abs(cov - ecov)):.3g} "
          f"(bound {FIT_COV_ATOL:.3g})")
    assert np.max(np.abs(mu - emu)) <= FIT_MU_ATOL and np.max(np.abs(cov - ecov)) <= FIT_COV_ATOL
    # saved, reloaded and used through pyiqa.create_metric on a (1, 3, H, W) tensor: the same score as the ctypes handle
    path = str(tmp_path / "fitted.npz")
    iqa_mod.save_niqe_model(path, mu, cov + np.diag(np.diag(cov)) * 1e-3 + 1e-9 * np.eye(36))
    mu2, cov2 = iqa_mod.load_niqe_model(path)
    compat.install()
    import pyiqa
    metric = pyiqa.create_metric("niqe", device=torch.device("cuda"), pretrained_model_path=path)
    rgb = np.ascontiguousarray(np.moveaxis(_rgb("det_photo4k").astype(np.float32) / np.float32(255), 2, 0))
    want = iqa.niqe([rgb], mu2, cov2)
    for t in (torch.from_numpy(rgb)[None], torch.from_numpy(rgb)[None].cuda(), torch.from_numpy(rgb)):
        got = metric(t)
        assert got.shape == (1,) and got.dtype == torch.float32 and got.device == t.device
        assert got.item() == np.float32(want[0])
    both = metric(torch.from_numpy(np.stack([rgb, rgb[:, ::-1].copy()])).cuda())
    assert both.shape == (2,) and both[0].item() == np.float32(want[0]) and both[1].item() != both[0].item()
    assert metric(rgb).item() == np.float32(want[0]) and metric(np.moveaxis(rgb, 0, 2)).item() == np.float32(want[0])


def measure():
    """The float32 oracle against the float64 oracle on this file's inputs: where the tolerances in the header come from."""
    cs = cases()
    f64 = {k: R.features(v) for k, v in cs.items()}
    fe = sh = naive = 0.0
    apart = total = 0
    rest = [c for c in range(36) if c not in ALPHA_COLS]
    f32 = {}
    for k, v in cs.items():
        f32[k] = R.features(v, np.float32)
        a64, a32 = R.alphas_of(f64[k][0]), R.alphas_of(f32[k][0])
        apart, total = apart + int(np.count_nonzero(a64 != a32)), total + a64.size
        at = R.features(v, np.float32, alpha=a64)
        fe = max(fe, np.nanmax(np.abs(at[0][:, rest] - f64[k][0][:, rest])))
        sh = max(sh, np.max(np.abs(at[1] - f64[k][1]) / f64[k][1]))
        nv = R.features_from_luma(R.luma(v), np.float32, alpha=a64, shifted=False)[0]
        naive = max(naive, np.nanmax(np.abs(nv[:, rest] - f64[k][0][:, rest])))
    mu, cov = pristine_model(np.concatenate([f64[k][0] for k in cs]))
    sc = max(abs(R.score(f32[k][0], mu, cov) - R.score(f64[k][0], mu, cov)) / R.score(f64[k][0], mu, cov) for k in cs)
    nan64, nan32 = R.features(nan_image()), R.features(nan_image(), np.float32)
    mu2, cov2 = pristine_model(f64["family_224x320"][0])
    sc = max(sc, abs(R.score(nan32[0], mu2, cov2) - R.score(nan64[0], mu2, cov2)) / R.score(nan64[0], mu2, cov2))
    det64 = [R.features(_gray(n)) for n in DET]
    det32 = [R.features(_gray(n), np.float32, alpha=R.alphas_of(f[0])) for n, f in zip(DET, det64)]
    (m64, c64), (m32, c32) = R.fit(det64), R.fit(det32)
    print(f"features  {fe:.3g} x8 = {8 * fe:.3g}   (naive float32 form: {naive:.3g})")
    print(f"sharpness {sh:.3g} x8 = {8 * sh:.3g}")
    print(f"score     {sc:.3g} x8 = {8 * sc:.3g}")
    print(f"fit mu    {np.max(np.abs(m32 - m64)):.3g} x8 = {8 * np.max(np.abs(m32 - m64)):.3g}; cov {np.max(np.abs(c32 - c64)):.3g} x8 = {8 * np.max(np.abs(c32 - c64)):.3g}")
    print(f"shapes apart: {apart} of {total}")


if __name__ == "__main__":
    measure()
