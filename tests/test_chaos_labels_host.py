"""CPU checks of the device route for the chaos labels: the C ABI entry, the Python options in front of it (dataset `labels`,
get_chaos_features' `as_tensor`, train.py's configuration key) and the index builder of chunk_chaos_labels_device.  No kernel runs."""
import inspect
import os
import re

import numpy as np
import pytest

from smokephysai_amd import _lib
from smokephysai_amd.physics import SmokeSimulator
from smokephysai_amd.utils import data_loader
from smokephysai_amd.utils.data_loader import HIST_TAIL, SyntheticSmokeDataset, chaos_label_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chaos_features_declared_exported_bound():
    hdr = open(os.path.join(ROOT, "include", "smokehip.h")).read()
    L = _lib.load()
    assert re.search(r"\bsmk_chaos_features\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "smk_chaos_features" in _lib.EXPORTS and hasattr(L, "smk_chaos_features")
    assert len(L.smk_chaos_features.argtypes) == 11
    assert int(re.search(r"#define\s+SMK_ABI_VERSION\s+(\d+)", hdr).group(1)) == 17 == _lib.ABI_VERSION == L.smk_abi_version()


def test_chaos_features_checks_arguments_before_any_device_work():
    L = _lib.load()
    a = 4096                                                                   # an aligned stand-in address: never dereferenced
    assert L.smk_chaos_features(None, None, None, 4, None, None, 1, 0, None, None, None) == -1      # null pointers
    assert L.smk_chaos_features(a, a, a, 0, a, a, 1, 0, a, None, None) == -1                        # S < 1
    assert L.smk_chaos_features(a, a, a, 4, a, a, 0, 0, a, None, None) == -1                        # F < 1
    assert L.smk_chaos_features(None, a, a, 4, a, a, 1, 0, a, None, None) == -1                     # norms missing with S > 1
    assert L.smk_chaos_features(a, a, a + 4, 4, a, a, 1, 0, a, None, None) == -1                    # hist not 16-byte aligned
    assert L.smk_chaos_features(a, a, a, 4, a, a, 10, 3, a, a, None) == -1                          # groups do not divide F
    assert L.smk_chaos_features(a, a, a, 4, a, a, 10, 5, a, None, None) == -1                       # groups without means


def test_dataset_labels_option_is_keyword_only_and_validated_without_a_gpu():
    p = inspect.signature(SyntheticSmokeDataset.__init__).parameters["labels"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "host"
    with pytest.raises(ValueError, match="labels"):
        SyntheticSmokeDataset(num_samples=1, grid_size=(64, 64), labels="bogus")
    with pytest.raises(ValueError, match="labels"):
        SyntheticSmokeDataset(num_samples=1, grid_size=(64, 64), device="cpu", labels="gpu")      # ... before the device check


def test_get_chaos_features_has_as_tensor_default_false():
    p = inspect.signature(SmokeSimulator.get_chaos_features).parameters["as_tensor"]
    assert p.default is False


def _config(hw=None):
    cfg = {"training": {"batch_size": 4}, "data": {"num_train": 6, "num_val": 2, "grid_size": [64, 64], "cache_dir": None}}
    if hw is not None:
        cfg["mi355x"] = hw
    return cfg


def test_train_forwards_dataset_labels():
    import train
    import yaml
    assert train.data_loader_kwargs(_config())["labels"] == "host"                         # no mi355x section
    assert train.data_loader_kwargs(_config({}))["labels"] == "host"                       # empty section
    assert train.data_loader_kwargs(_config({"sim_batch": 8}))["labels"] == "host"         # section without the key
    kw = train.data_loader_kwargs(_config({"dataset_labels": "device", "sim_batch": 8, "jacobi_iters": 10}), rank=1, world=2)
    assert kw == dict(batch_size=4, num_train=6, num_val=2, grid_size=(64, 64), cache_dir=None, sim_batch=8, jacobi_iters=10,
                      labels="device", rank=1, world=2)
    # every key is one create_data_loaders or SyntheticSmokeDataset accepts
    accepted = set(inspect.signature(data_loader.create_data_loaders).parameters) | set(inspect.signature(SyntheticSmokeDataset.__init__).parameters)
    assert set(kw) <= accepted
    # a bad value reaches the dataset's own check (and fails there without a GPU)
    bad = train.data_loader_kwargs(_config({"dataset_labels": "numpy"}))
    with pytest.raises(ValueError, match="labels"):
        data_loader.create_data_loaders(device="cuda", **bad)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "config.yaml")))
    assert cfg["mi355x"]["dataset_labels"] == "host"
    assert train.data_loader_kwargs(cfg)["labels"] == "host"


def _rows_from_labels_from_stats(n, T, valid_head, start=10):
    """labels_from_stats' window arithmetic inside chunk_chaos_labels' slicing, transcribed: for every row the buffer index of its
    frame, the buffer indices of the first and one-past-last distance of its Lyapunov window (None below 20 frames), and whether the
    row exists at all (history of at least 10)."""
    rows = []
    for i in range(n):
        off = min(HIST_TAIL, valid_head + i * T)
        lo = HIST_TAIL + i * T - off                       # d handed to labels_from_stats starts at buffer distance `lo`
        for t in range(start, T):
            e = off + t
            assert e + 1 >= 10
            win = (lo + e - 19, lo + e) if e + 1 >= 20 else None
            rows.append((HIST_TAIL + i * T + t, win))      # box / hist row: frame i * T + t of buf[HIST_TAIL:]
    return rows


@pytest.mark.parametrize("valid_head", [0, 5, 19])
@pytest.mark.parametrize("T", [12, 20, 25])
@pytest.mark.parametrize("n", [1, 3])
def test_label_rows_match_the_host_window_arithmetic(valid_head, T, n):
    pos, hist_len = chaos_label_rows(n, T, valid_head)
    want = _rows_from_labels_from_stats(n, T, valid_head)
    assert pos.dtype == hist_len.dtype == np.int32 and pos.shape == hist_len.shape == (len(want),) == (n * (T - 10),)
    for k, (frame, win) in enumerate(want):
        assert pos[k] == frame
        assert (hist_len[k] >= 20) == (win is not None) and hist_len[k] >= 10
        if win is not None:                                # the kernel reads norms[pos-19 .. pos-1]
            assert (pos[k] - 19, pos[k]) == win and win[0] >= HIST_TAIL - valid_head and win[0] >= 0
        assert pos[k] < HIST_TAIL + n * T


def test_label_rows_corners():
    pos, hist_len = chaos_label_rows(2, 10, 0)             # T <= start: no rows
    assert pos.shape == hist_len.shape == (0,)
    pos, hist_len = chaos_label_rows(1, 20, 0, start=9)
    assert hist_len[0] == 10 and pos[0] == HIST_TAIL + 9
