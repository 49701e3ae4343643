"""TEST INFRASTRUCTURE -- golden statistics of a freshly constructed UNMODIFIED reference model
(model/score_network.py ScoreNetwork, config/base.yaml with 2 IPA blocks, torch.manual_seed(0)).

Run in the build container only (needs the reference checkout):
    python oracle/make_golden_init.py
Writes tests/golden/init_stats.json: {state_dict key: [std, mean]} of every parameter / buffer, which
tests/test_init_and_checkpoint.py compares with this repository's ScoreNetwork under the same seed.
Must run in its own process: the reference's top-level package names (model, data) are generic.
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader as rl  # noqa: E402
from oracle.make_golden import GOLD  # noqa: E402


def main():
    rl.install()
    from model import score_network
    torch.manual_seed(0)
    m = score_network.ScoreNetwork(rl.base_conf(os.path.join(ROOT, "build", "igso3_cache"), num_blocks=2).model, None)
    stats = {k: [float(v.float().std()) if v.numel() > 1 else 0.0, float(v.float().mean())] for k, v in m.state_dict().items()}
    path = os.path.join(GOLD, "init_stats.json")
    with open(path, "w") as f:
        json.dump(stats, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {path}: {len(stats)} tensors")


if __name__ == "__main__":
    main()
