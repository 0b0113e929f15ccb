"""NIQE's pristine model: load it, fit it, save it.

The score (`_lib.IQA.niqe`) measures an image's block features against a 36-vector and a 36x36 matrix fitted to pristine images.
pyiqa ships them as `niqe_modelparameters.mat` (keys `mu_prisparam`, `cov_prisparam`); this build ships none and fetches none:
drop that file in, or fit a model from your own pristine images with `fit_niqe_model`.
"""
from __future__ import annotations

import os
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib

MODEL_FILE = "niqe_modelparameters.mat"
ENV_VAR = "FFP_NIQE_PARAMS"
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def search_paths(pretrained_model_path: Optional[str] = None) -> list:
    """Where the pristine model is looked for, in order: the caller's path, $FFP_NIQE_PARAMS, pyiqa's cache, models/."""
    out = []
    if pretrained_model_path:
        out.append(os.fspath(pretrained_model_path))
    if os.environ.get(ENV_VAR):
        out.append(os.environ[ENV_VAR])
    out.append(os.path.join(os.path.expanduser("~"), ".cache", "torch", "hub", "pyiqa", MODEL_FILE))
    out.append(os.path.join("models", MODEL_FILE))
    return out


def find_niqe_model(pretrained_model_path: Optional[str] = None) -> str:
    paths = search_paths(pretrained_model_path)
    for p in paths:
        if os.path.isfile(p):
            return p
    raise FileNotFoundError(
        f"NIQE needs its pristine model, {MODEL_FILE} (keys mu_prisparam, cov_prisparam), and none was found at: " + ", ".join(paths) +
        f". Copy pyiqa's file to one of these places (or name it with pretrained_model_path= or ${ENV_VAR}), or fit a model from your "
        "own pristine images with ffp_amd.iqa.fit_niqe_model and save it with save_niqe_model. Nothing is downloaded.")


def load_niqe_model(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """(mu [36], cov [36, 36]) float64 from a .mat (scipy.io.loadmat) or .npz file with keys mu_prisparam, cov_prisparam."""
    path = os.fspath(path)
    if path.lower().endswith(".npz"):
        with np.load(path) as z:
            d = {k: z[k] for k in z.files}
    else:
        from scipy.io import loadmat
        d = loadmat(path)
    for k in ("mu_prisparam", "cov_prisparam"):
        if k not in d:
            raise ValueError(f"{path}: no '{k}' in the file (found {sorted(k for k in d if not k.startswith('__'))})")
    mu = np.asarray(d["mu_prisparam"], np.float64).reshape(-1)
    cov = np.asarray(d["cov_prisparam"], np.float64)
    if mu.shape != (_lib.NIQE_FEATURES,) or cov.shape != (_lib.NIQE_FEATURES, _lib.NIQE_FEATURES):
        raise ValueError(f"{path}: expected a 36-vector and a 36x36 matrix, got {mu.shape} and {cov.shape}")
    return mu, cov


def save_niqe_model(path: str, mu: np.ndarray, cov: np.ndarray) -> None:
    """The .npz form of the model (np.savez appends .npz to a path without it)."""
    np.savez(os.fspath(path), mu_prisparam=np.asarray(mu, np.float64).reshape(1, -1), cov_prisparam=np.asarray(cov, np.float64))


def fit_niqe_model(images: Sequence[np.ndarray], sharpness_threshold: float = 0.75, device: int = 0, chan_order: int = _lib.CHAN_AS_RGB,
                   engine: Optional[_lib.IQA] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The training step of Mittal et al. 2013 on pristine images (forms as _lib.IQA.niqe_features takes them): per image the
    blocks whose sharpness exceeds `sharpness_threshold` times the image's maximum, then the mean and the sample covariance of
    the 36 features of all kept blocks (blocks with a NaN feature are left out). Features come from the device."""
    q = engine or _lib.IQA(device)
    try:
        feat, sharp, off = q.niqe_features(images, chan_order)
    finally:
        if engine is None:
            q.close()
    keep = []
    for i in range(len(off) - 1):
        f, s = feat[off[i]:off[i + 1]].astype(np.float64), sharp[off[i]:off[i + 1]]
        f = f[s > sharpness_threshold * s.max()]
        keep.append(f[~np.isnan(f).any(axis=1)])
    X = np.concatenate(keep)
    if X.shape[0] < 2:
        raise ValueError(f"{X.shape[0]} block(s) kept: a covariance needs at least two")
    return X.mean(axis=0), np.cov(X, rowvar=False)
