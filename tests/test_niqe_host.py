"""CPU tests of NIQE: known answers of the oracle (tests/niqe_ref.py), the host-side score of the C-ABI against it, the pristine
model's files and search order, and the pyiqa shim's boundary (nothing here touches a GPU)."""
import os

import numpy as np
import pytest

import niqe_ref as R


@pytest.fixture(scope="module")
def lib():
    from ffp_amd import _lib, build
    build.build(verbose=False)
    _lib.lib()
    return _lib


@pytest.fixture()
def pyiqa():
    import ffp_amd.compat as compat
    compat.install()
    import pyiqa
    if not getattr(pyiqa, "__version__", "").endswith("ffp-shim"):
        pytest.fail("a real pyiqa is installed: these tests are about the shim")
    return pyiqa


def _model(seed=0):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((36, 36))
    return rng.standard_normal(36), a @ a.T / 36 + 0.1 * np.eye(36)


# ---- oracle known answers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_aggd_recovers_gaussian_and_laplacian_shape(dtype):
    """Two grid steps (0.002) is far below the sampling error of 1e5 random draws (the estimate's sd is about 0.015), so the samples
    are the distribution's 1e5 mid-point quantiles: drawn without sampling noise."""
    from scipy.stats import laplace, norm
    p = (np.arange(100000) + 0.5) / 100000
    a, l, r = R.aggd(norm.ppf(p), dtype)[:3]
    assert abs(a - 2.0) <= 0.002 + 1e-12, a
    assert abs(l / r - 1) < 1e-6
    a = R.aggd(laplace.ppf(p), dtype)[0]
    assert abs(a - 1.0) <= 0.002 + 1e-12, a


def test_aggd_shape_on_exact_moment_ratio():
    """Samples are noisy; the table is not: a ratio taken from the table itself comes back as its own grid point."""
    for i in (0, 800, 1800, 9800):
        assert int(np.argmin((R.R_GAM - R.R_GAM[i]) ** 2)) == i
    assert np.all(np.diff(R.R_GAM) > 0)                  # monotone: what lets the device bisect
    assert abs(R.GAM[1800] - 2.0) < 1e-12 and abs(R.R_GAM[1800] - 2 / np.pi) < 1e-12      # Gaussian: E|x|^2 / E x^2 = 2 / pi
    assert abs(R.R_GAM[800] - 0.5) < 1e-12               # Laplacian


@pytest.mark.parametrize("n", [96, 192, 97, 288])
def test_resize_matrix_rows_sum_to_one(n):
    m = R.resize_matrix(n)
    assert m.shape == ((n + 1) // 2, n)
    np.testing.assert_allclose(m.sum(1), 1.0, atol=1e-14)


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-12), (np.float32, 1e-4)])
def test_constant_image_resizes_to_itself(dtype, tol):
    out = R.half_size(np.full((96, 192), 137.0), dtype)
    assert out.shape == (48, 96)
    np.testing.assert_allclose(out, 137.0, atol=tol)


def test_half_size_interior_taps():
    j, w = R.resize_taps(96)
    assert j[10].tolist() == list(range(17, 27))         # taps 2i-3 .. 2i+6
    assert w[10, 8] == 0 and w[10, 9] == 0 and abs(w[10, 3] - w[10, 4]) < 1e-15      # symmetric about u = 2i + 0.5
    assert j[0].tolist()[:3] == [2, 1, 0]                # -3, -2, -1 reflect with the edge pixel repeated


def test_flat_block_is_nan_where_the_arithmetic_is():
    f = R.block_features(np.zeros((96, 96)))
    assert f[0] == 0.2 and np.isnan(f[1]) and all(np.isnan(f[k]) for k in (3, 4, 5))


# ---- the host half of the C-ABI ----------------------------------------------------------------------------------------------------
def test_score_matches_oracle(lib):
    rng = np.random.default_rng(3)
    mu, cov = _model()
    f1 = (mu + 0.7 * rng.standard_normal((60, 36))).astype(np.float64)
    f2 = (mu + 0.3 * rng.standard_normal((9, 36))).astype(np.float64)      # fewer blocks than features: C is singular, the sum is not
    f2[4, 7] = np.nan
    off = np.asarray([0, 60, 69], np.int64)
    got = lib.niqe_score(np.concatenate([f1, f2]), off, mu, cov)
    want = [R.score(f1, mu, cov), R.score(f2, mu, cov)]
    np.testing.assert_allclose(got, want, rtol=1e-9)


def test_score_pinv_drops_the_null_space(lib):
    rng = np.random.default_rng(4)
    v = rng.standard_normal((36, 5))
    cov = v @ v.T                                        # rank 5; with 4 blocks the sum has rank <= 8
    f = rng.standard_normal((4, 36))
    got = lib.niqe_score(f, np.asarray([0, 4], np.int64), np.zeros(36), cov)
    assert np.isfinite(got[0])
    np.testing.assert_allclose(got[0], R.score(f, np.zeros(36), cov), rtol=1e-6)


def test_score_rejects_bad_arguments(lib):
    mu, cov = _model()
    with pytest.raises(ValueError):
        lib.niqe_score(np.zeros((4, 36)), np.asarray([0, 3], np.int64), mu, cov)
    with pytest.raises(ValueError):
        lib.niqe_score(np.zeros((4, 36)), np.asarray([0, 4], np.int64), mu[:35], cov)
    assert np.isnan(lib.niqe_score(np.zeros((1, 36)), np.asarray([0, 1], np.int64), mu, cov)[0])
    assert lib.niqe_blocks(200, 300) == 6 and lib.niqe_blocks(95, 4000) == 0


# ---- the pristine model's files ----------------------------------------------------------------------------------------------------
def test_model_mat_npz_round_trip(tmp_path, lib):
    from scipy.io import savemat
    from ffp_amd import iqa
    mu, cov = _model(5)
    savemat(tmp_path / "niqe_modelparameters.mat", {"mu_prisparam": mu.reshape(1, -1), "cov_prisparam": cov})
    m1, c1 = iqa.load_niqe_model(str(tmp_path / "niqe_modelparameters.mat"))
    iqa.save_niqe_model(str(tmp_path / "again.npz"), m1, c1)
    m2, c2 = iqa.load_niqe_model(str(tmp_path / "again.npz"))
    for m, c in ((m1, c1), (m2, c2)):
        assert m.shape == (36,) and c.shape == (36, 36) and m.dtype == np.float64
        assert np.array_equal(m, mu) and np.array_equal(c, cov)
    np.savez(tmp_path / "bad.npz", mu_prisparam=mu)
    with pytest.raises(ValueError, match="cov_prisparam"):
        iqa.load_niqe_model(str(tmp_path / "bad.npz"))
    np.savez(tmp_path / "short.npz", mu_prisparam=mu[:18], cov_prisparam=cov)
    with pytest.raises(ValueError, match="36"):
        iqa.load_niqe_model(str(tmp_path / "short.npz"))


def test_model_search_order(tmp_path, monkeypatch, lib):
    from ffp_amd import iqa
    home, cwd = tmp_path / "home", tmp_path / "cwd"
    cache = home / ".cache" / "torch" / "hub" / "pyiqa"
    for d in (cache, cwd / "models", tmp_path / "kw", tmp_path / "env"):
        d.mkdir(parents=True)
    monkeypatch.setenv("HOME", str(home))
    monkeypatch.chdir(cwd)
    monkeypatch.delenv("FFP_NIQE_PARAMS", raising=False)
    mu, cov = _model()
    places = [tmp_path / "kw" / "k.npz", tmp_path / "env" / "e.npz", cache / "niqe_modelparameters.mat", cwd / "models" / "niqe_modelparameters.mat"]
    with pytest.raises(FileNotFoundError) as e:
        iqa.find_niqe_model(None)
    assert "niqe_modelparameters.mat" in str(e.value) and "fit_niqe_model" in str(e.value)
    for p in reversed(places):                           # each place added outranks the ones already there
        if p.suffix == ".npz":
            iqa.save_niqe_model(str(p), mu, cov)
        else:
            p.write_bytes(b"x")
        if p.parent.name == "env":
            monkeypatch.setenv("FFP_NIQE_PARAMS", str(p))
        kw = str(places[0]) if p == places[0] else None
        assert os.path.abspath(iqa.find_niqe_model(kw)) == str(p)
    assert iqa.search_paths(str(places[0]))[:2] == [str(places[0]), str(places[1])]


# ---- the pyiqa shim ----------------------------------------------------------------------------------------------------------------
def test_shim_names_what_is_missing(tmp_path, monkeypatch, pyiqa):
    monkeypatch.setenv("HOME", str(tmp_path))
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("FFP_NIQE_PARAMS", raising=False)
    with pytest.raises(FileNotFoundError) as e:
        pyiqa.create_metric("niqe", device="cuda")
    assert "niqe_modelparameters.mat" in str(e.value) and "fit_niqe_model" in str(e.value)
    with pytest.raises(FileNotFoundError):
        pyiqa.create_metric("niqe", device="cuda", pretrained_model_path=str(tmp_path / "nowhere.mat"))
    with pytest.raises(NotImplementedError, match="BRISQUE is not built"):
        pyiqa.create_metric("brisque", device="cuda")
    with pytest.raises(NotImplementedError, match="only 'niqe'"):
        pyiqa.create_metric("topiq_nr-face")
    assert pyiqa.list_models() == ["niqe"]


def test_shim_metric_attributes_and_too_small_image(tmp_path, monkeypatch, pyiqa):
    import torch
    from ffp_amd import iqa
    mu, cov = _model()
    iqa.save_niqe_model(str(tmp_path / "m.npz"), mu, cov)
    monkeypatch.setenv("FFP_NIQE_PARAMS", str(tmp_path / "m.npz"))
    m = pyiqa.create_metric("niqe", device=torch.device("cpu"))          # found through the environment; no GPU is touched
    assert m.metric_name == "niqe" and m.lower_better is True and m.metric_mode == "NR"
    assert np.array_equal(m.mu, mu) and m.model_path == str(tmp_path / "m.npz")
    for bad in (torch.zeros(1, 3, 96, 191), torch.zeros(3, 95, 400), np.zeros((100, 100, 3), np.float32), np.zeros((96, 96), np.float32)):
        with pytest.raises(ValueError, match="two 96x96 blocks"):
            m(bad)
    with pytest.raises(ValueError):
        m(torch.zeros(1, 2, 192, 192))
    with pytest.raises(NotImplementedError):
        pyiqa.create_metric("niqe", as_loss=True)
