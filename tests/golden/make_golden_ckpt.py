"""Generate tests/golden/reference_checkpoints.npz from the reference's shipped DDPG artefacts (build container only; see
make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ckpt.py <reference tree>

For every task under <reference tree>/resources/DDPG/: the actor.pth / critic.pth state_dicts (key names in order, every
tensor's shape and its float32 values) and the text of obs.yaml / dg.yaml, so that tests/test_reference_artifacts.py needs
nothing outside the repository.  A tensor of more than SAMPLE_ABOVE entries keeps SAMPLE of its values at fixed seeded flat
positions (the larger weight matrices; whole, they would make a file of more than 1 MB); the test fills the other positions
with seeded values.
Layout: `tasks` (names), `<task>__<net>__keys` (the state_dict's keys), `<task>__<net>__<i>__shape`, `<task>__<net>__<i>` (the
i-th tensor's values, all of them or the sample), `<task>__<net>__<i>__idx` (the sample's flat positions, sampled tensors only),
`<task>__<file>` (the yaml text)."""
import glob
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
SAMPLE_ABOVE = 1024
SAMPLE = 512


def main(ref_root):
    base = os.path.join(ref_root, "resources", "DDPG")
    tasks = sorted(os.path.basename(p) for p in glob.glob(os.path.join(base, "*")) if os.path.isdir(p))
    assert tasks, f"no task directories under {base}"
    out = dict(tasks=np.array(tasks))
    gen = np.random.default_rng(1898)
    for task in tasks:
        for net in ("actor", "critic"):
            sd = torch.load(os.path.join(base, task, net + ".pth"), map_location="cpu", weights_only=True)
            out[f"{task}__{net}__keys"] = np.array(list(sd.keys()))
            for i, v in enumerate(sd.values()):
                flat = v.numpy().astype(np.float32).reshape(-1)
                out[f"{task}__{net}__{i}__shape"] = np.array(v.shape, dtype=np.int64)
                if flat.size > SAMPLE_ABOVE:
                    idx = np.sort(gen.choice(flat.size, size=SAMPLE, replace=False)).astype(np.uint16 if flat.size <= 1 << 16 else np.int32)
                    out[f"{task}__{net}__{i}__idx"] = idx
                    flat = flat[idx]
                out[f"{task}__{net}__{i}"] = flat
        for fname in ("obs.yaml", "dg.yaml"):
            with open(os.path.join(base, task, fname)) as f:
                out[f"{task}__{fname}"] = np.array(f.read())
    path = os.path.join(HERE, "reference_checkpoints.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", ", ".join(tasks))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
