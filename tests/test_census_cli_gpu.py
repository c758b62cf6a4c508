"""GPU (MI355X): the census through the command-line tools, in process, on six synthetic episodes: a ``tools/train.py`` run with a
``val_census:`` block writes ``val/latent/*`` into ``metrics.jsonl``, and ``tools/latent_census.py`` prints the per-categorical table of
the checkpoint that run wrote and writes it as JSON."""

from __future__ import annotations

import json
import math
import sys

import numpy as np
import pytest

import multimodal_mtrssm_amd as mt

pytestmark = pytest.mark.gpu

KEYS = ("post_entropy", "prior_entropy", "kl", "perplexity", "mi", "prior_gap", "switch_rate", "unused", "active")


def test_train_logs_the_census_and_the_cli_prints_the_table_of_its_checkpoint(tmp_path, monkeypatch, capsys) -> None:  # noqa: ANN001
    sys.path.insert(0, str(mt._lib._HERE.parent / "tools"))  # noqa: SLF001
    import latent_census
    import train

    rng = np.random.default_rng(5)
    (tmp_path / "data").mkdir()
    for i, n in enumerate((8, 8, 9, 8, 10, 8)):
        np.savez(tmp_path / "data" / f"ep{i}.npz", audio=rng.uniform(-80.0, 0.0, (n, 32, 32)).astype(np.float32),
                 image=rng.uniform(0.0, 255.0, (n, 1, 32, 32)).astype(np.float32), label=rng.integers(-1, 10, n).astype(np.int64),
                 speaker=np.eye(6, dtype=np.float32)[np.full(n, i)])
    dims = (8, 8, 4, 2, 16)
    config = {"model": "mrssm", "dims": list(dims),
              "trainer": {"batch_size": 2, "steps": 8, "scheduler": None, "early_stopping": None,
                          "val_census": {"observe": ["both", "audio"], "active_nats": 0.02}}}
    (tmp_path / "train.json").write_text(json.dumps(config))
    run = tmp_path / "run"
    monkeypatch.setattr(sys, "argv", ["train.py", "--config", str(tmp_path / "train.json"), "--data-dir", str(tmp_path / "data"), "--out", str(run),
                                      "--epochs", "2"])
    train.main()
    capsys.readouterr()
    lines = [json.loads(x) for x in (run / "metrics.jsonl").read_text().splitlines()]
    want = {f"val/latent/{o}/{k}" for o in ("both", "audio") for k in KEYS} | {"val/latent/audio/cross"}
    assert len(lines) == 2 and all(want <= set(line) for line in lines)  # noqa: PLR2004
    assert all(math.isfinite(line[k]) for line in lines for k in want)
    first = lines[0]
    assert 0.0 < first["val/latent/both/post_entropy"] <= math.log(4) + 1e-6 and 1.0 <= first["val/latent/both/perplexity"] <= 4.0 + 1e-6  # noqa: PLR2004
    assert 0.0 <= first["val/latent/both/unused"] <= 8.0 and 0.0 <= first["val/latent/audio/active"] <= 2.0 and first["val/latent/audio/cross"] >= 0.0  # noqa: PLR2004

    out = tmp_path / "census.json"
    monkeypatch.setattr(sys, "argv", ["latent_census.py", "--checkpoint", str(run / "last.ckpt"), "--data-dir", str(tmp_path / "data"),
                                      "--dims", ",".join(map(str, dims)), "--window", "6", "--batch", "4", "--observe", "both,vision", "--json", str(out)])
    latent_census.main()
    printed = capsys.readouterr().out
    assert "Latent census: MoPoE-MRSSM" in printed and "posterior observes both: 51 live frames" in printed and "posterior observes vision" in printed
    for col in ("perplexity", "unused", "kl", "active", "mi", "prior_gap", "switch_rate", "dwell", "cross", "usage"):
        assert col in printed, col
    tree = json.loads(out.read_text())
    assert tree["observe"] == ["both", "vision"] and tree["windows"] == 12 and tree["steps"] == 6 and list(tree["levels"]) == ["latent"]  # noqa: PLR2004
    level = tree["levels"]["latent"]
    assert level["categoricals"] == 2 and level["classes"] == 4 and level["frames"] == [51.0, 51.0]  # noqa: PLR2004
    both, vision = level["groups"]["both"], level["groups"]["vision"]
    assert both["cross"] == [0.0, 0.0] and all(x > 0.0 for x in vision["cross"])
    assert len(both["usage"]) == 2 and all(abs(sum(u) - 1.0) < 1e-12 for u in both["usage"]) and len(both["by_position"]["kl"]) == 6  # noqa: PLR2004
    assert all(x is not None for key in ("perplexity", "kl", "mi", "prior_gap", "switch_rate", "dwell") for x in both[key])
