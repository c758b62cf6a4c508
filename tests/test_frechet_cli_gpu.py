"""GPU (MI355X): ``tools/frechet_distance.py`` in process, on six synthetic episodes: the checkpoint of a short ``tools/train.py`` run
and a saved ``DigitClassifier`` give the table per stream and bin, printed and as JSON, with the hand-counted rows per bin."""

from __future__ import annotations

import json
import sys

import numpy as np
import pytest
import torch

import multimodal_mtrssm_amd as mt

pytestmark = pytest.mark.gpu


def test_the_cli_prints_the_table_of_a_checkpoint(tmp_path, monkeypatch, capsys) -> None:  # noqa: ANN001
    sys.path.insert(0, str(mt._lib._HERE.parent / "tools"))  # noqa: SLF001
    import frechet_distance
    import train

    rng = np.random.default_rng(5)
    (tmp_path / "data").mkdir()
    for i, n in enumerate((8, 8, 9, 8, 10, 8)):
        np.savez(tmp_path / "data" / f"ep{i}.npz", audio=rng.uniform(-80.0, 0.0, (n, 32, 32)).astype(np.float32),
                 image=rng.uniform(0.0, 255.0, (n, 1, 32, 32)).astype(np.float32), label=rng.integers(-1, 10, n).astype(np.int64),
                 speaker=np.eye(6, dtype=np.float32)[np.full(n, i)])
    dims = (8, 8, 4, 2, 16)
    config = {"model": "mrssm", "dims": list(dims), "trainer": {"batch_size": 2, "steps": 8, "scheduler": None, "early_stopping": None}}
    (tmp_path / "train.json").write_text(json.dumps(config))
    run = tmp_path / "run"
    monkeypatch.setattr(sys, "argv", ["train.py", "--config", str(tmp_path / "train.json"), "--data-dir", str(tmp_path / "data"), "--out", str(run),
                                      "--epochs", "1"])
    train.main()
    with torch.random.fork_rng():
        torch.manual_seed(3)
        torch.save(mt.DigitClassifier().state_dict(), tmp_path / "mnist_cnn.pt")
    capsys.readouterr()

    # windows of 6 frames: six whole ones and the tails 2, 2, 3, 2, 4, 2 -- 51 live frames; a context of 2 and the edges (1, 2)
    counts = {"obs": 24.0, "h1": 8.0, "h2": 19.0}
    base = ["frechet_distance.py", "--checkpoint", str(run / "last.ckpt"), "--data-dir", str(tmp_path / "data"), "--dims", ",".join(map(str, dims)),
            "--window", "6", "--batch", "4", "--query", "2", "--samples", "3", "--edges", "1,2"]
    for features, streams, dim, extra in (("reader", ["vision"], 128, ["--classifier", str(tmp_path / "mnist_cnn.pt")]),
                                          ("encoder", ["audio", "vision"], 16, [])):
        out = tmp_path / f"{features}.json"
        monkeypatch.setattr(sys, "argv", [*base, "--features", features, "--json", str(out), *extra])
        frechet_distance.main()
        printed = capsys.readouterr().out
        assert "Frechet distance: MoPoE-MRSSM, 12 windows of up to 6 frames" in printed and f"({dim} features)" in printed
        for col in ("fd", "mean", "cov", "trace_ratio", "n_real", "n_generated", "obs", "h1", "h2"):
            assert col in printed, col
        tree = json.loads(out.read_text())
        assert tree["windows"] == 12 and tree["features"] == dim and tree["bins"] == ["obs", "h1", "h2"] and list(tree["streams"]) == streams  # noqa: PLR2004
        for stream in streams:
            for name, n in counts.items():
                row = tree["streams"][stream][name]
                assert row["n_real"] == n and row["n_generated"] == 3 * n, (stream, name, row)
                assert row["fd"] is not None and row["fd"] >= 0.0 and row["mean"] >= 0.0 and row["trace_ratio"] > 0.0, (stream, name, row)
    monkeypatch.setattr(sys, "argv", [*base, "--features", "reader"])
    with pytest.raises(SystemExit):
        frechet_distance.main()  # (the reader needs --classifier)
