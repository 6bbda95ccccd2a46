"""train.py --device-store as a user runs it: one epoch of training and the evaluation on the committed mini dataset, fed by
drn_amd.store.StoreLoader, in a process of its own."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_train_py_runs_an_epoch_from_the_device_store(tmp_path):
    import yaml
    from test_store_gpu import MINI, mini_cfg
    cfg = dict(mini_cfg(3), batch_size=4, test_batch_size=4)
    config = tmp_path / "mini.yaml"
    config.write_text(yaml.safe_dump({"Charades": cfg}))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--root", MINI, "--config", str(config), "--stage", "3",
                          "--n-epoch", "1", "--device-store", "--workers", "0", "--snapshot-pref", str(tmp_path / "snap")],
                         cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert any(l.startswith("device store: 6 videos") for l in lines), lines
    rec = json.loads(lines[-1])
    assert rec["epoch"] == 0 and rec["train_loss"] == rec["train_loss"] and 0.0 <= rec["top1"] <= rec["top5"] <= 100.0
