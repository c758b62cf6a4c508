"""GPU (MI355X): ``tools/held_out_likelihood.py`` end to end, in process, on three synthetic episodes (one shorter than a window) and an
untrained model: the two bounds side by side, and at ``--threshold 0`` the particle filter's column is the importance-weighted one."""

from __future__ import annotations

import json
import math
import sys

import numpy as np
import pytest
import torch

import multimodal_mtrssm_amd as mt

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("threshold", [1.0, 0.0])
def test_held_out_likelihood_cli_prints_the_two_bounds(tmp_path, monkeypatch, capsys, threshold: float) -> None:  # noqa: ANN001
    sys.path.insert(0, str(mt._lib._HERE.parent / "tools"))  # noqa: SLF001
    import held_out_likelihood
    import word_transitions

    rng = np.random.default_rng(3)
    (tmp_path / "test").mkdir()
    for i, n in enumerate((12, 5, 7)):
        np.savez(tmp_path / "test" / f"ep{i}.npz", audio=rng.uniform(-80.0, 0.0, (n, 32, 32)).astype(np.float32),
                 image=rng.uniform(0.0, 255.0, (n, 1, 32, 32)).astype(np.float32), label=rng.integers(-1, 10, n).astype(np.int64),
                 speaker=np.eye(6, dtype=np.float32)[np.full(n, i)])
    dims = (8, 8, 4, 2, 16)
    torch.manual_seed(0)
    torch.save(word_transitions.build_model("mrssm", dims, "cpu").state_dict(), tmp_path / "model.ckpt")
    out = tmp_path / "results" / "held_out"
    monkeypatch.setattr(sys, "argv", ["held_out_likelihood.py", "--checkpoint", str(tmp_path / "model.ckpt"), "--data-dir", str(tmp_path / "test"),
                                      "--output", str(out), "--dims", ",".join(map(str, dims)), "--window", "6", "--batch", "3", "--samples", "4",
                                      "--resample-every", "2", "--threshold", str(threshold)])
    held_out_likelihood.main()
    printed = capsys.readouterr().out
    assert "| | importance-weighted (6k) | particle filter (6q) |" in printed and "| bound |" in printed
    res = json.loads(out.with_suffix(".json").read_text())
    assert res["frames"] == 24.0 and res["windows"] == 5 and res["samples"] == 4 and res["resample_every"] == 2  # noqa: PLR2004
    assert set(res["smc"]) == {f"smc/{k}" for k in ("smc", "mean", "audio", "vision", "latent", "ess", "resampled")}
    assert all(math.isfinite(v) for v in (*res["iw"].values(), *res["smc"].values()))
    assert len(res["smc_by_position"]["smc"]) == len(res["iw_by_position"]["iw"]) == 6  # noqa: PLR2004
    assert res["iw"]["loglik/iw"] >= res["iw"]["loglik/elbo"] and 1.0 <= res["smc"]["smc/ess"] <= 4.0  # noqa: PLR2004
    if threshold == 0.0:  # the same uniforms, nothing resampled: the same bound up to the loss-term tolerance
        assert res["smc"]["smc/resampled"] == 0.0
        np.testing.assert_allclose(res["smc"]["smc/smc"], res["iw"]["loglik/iw"], rtol=2e-5)
        np.testing.assert_allclose(res["smc"]["smc/mean"], res["iw"]["loglik/elbo"], rtol=2e-5)
    else:  # windows of 6, 6, 5, 6 and 1 frames, segments of 2: resampled after frames 1 and 3 of the windows that go on
        assert res["smc"]["smc/resampled"] == pytest.approx(8.0 / 24.0)
    assert "particle filter (6q)" in out.with_suffix(".md").read_text()
