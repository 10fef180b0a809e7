"""CPU: the checkpoint surface against the reference's own shipped artefacts (resources/DDPG/<task>/
{actor,critic}.pth, obs.yaml, dg.yaml), as captured in tests/golden/reference_checkpoints.npz
(tests/golden/make_golden_ckpt.py): state_dict keys in order, tensor shapes and values, and the yaml files' text.  The larger
weight matrices were stored as a fixed sample of their entries: the other entries are filled with seeded values, which the
round trip through the engine's flat layout must carry to the same positions like any others."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from conftest import GOLDEN

CKPT = np.load(os.path.join(GOLDEN, "reference_checkpoints.npz"), allow_pickle=False)
TASKS = [str(t) for t in CKPT["tasks"]]


def _tensor(task, net, i):
    shape = tuple(int(n) for n in CKPT[f"{task}__{net}__{i}__shape"])
    vals = CKPT[f"{task}__{net}__{i}"]
    if f"{task}__{net}__{i}__idx" not in CKPT.files:
        return vals.reshape(shape)
    full = np.random.default_rng(i).standard_normal(int(np.prod(shape))).astype(np.float32) * np.float32(vals.std())
    full[CKPT[f"{task}__{net}__{i}__idx"].astype(np.int64)] = vals
    return full.reshape(shape)


def _state_dict(task, net):
    keys = [str(k) for k in CKPT[f"{task}__{net}__keys"]]
    return OrderedDict((k, torch.from_numpy(_tensor(task, net, i))) for i, k in enumerate(keys))


@pytest.mark.parametrize("task", TASKS)
def test_state_dict_layout_matches_reference_checkpoints(gcrl, task):
    from gcrl_amd.src.model import Actor, Critic
    for fname, cls in (("actor.pth", Actor), ("critic.pth", Critic)):
        sd = _state_dict(task, fname[:-4])
        keys = list(sd.keys())
        first, last = sd[keys[0]], sd[keys[-2]]
        layers = len(keys) // 2 - 1                     # hidden Linear layers
        view = cls(None, fname, int(first.shape[1]), int(first.shape[0]), int(last.shape[0]), layers)
        layout = view._param_layout()
        assert [k for k, _ in layout] == keys                                   # names and order of module.parameters()
        assert [tuple(s) for _, s in layout] == [tuple(v.shape) for v in sd.values()]   # [out, in] weights
        flat = view.join(sd)                                                     # -> the engine's flat vector
        back = view.split(flat)
        for k in keys:
            assert np.array_equal(back[k], sd[k].numpy())


@pytest.mark.parametrize("task", TASKS)
def test_normaliser_yaml_loads(gcrl, task, tmp_path):
    from gcrl_amd.src.utils import RunningNormalizer
    for fname in ("obs.yaml", "dg.yaml"):
        path = tmp_path / fname
        path.write_text(str(CKPT[f"{task}__{fname}"]))
        import yaml
        raw = yaml.safe_load(open(path))
        n = RunningNormalizer(len(raw["mean"]))
        n.load(str(path))
        assert np.allclose(n.mean, np.asarray(raw["mean"], dtype=np.float64))
        x = np.zeros((2, len(raw["mean"])))
        assert np.all(np.abs(n.normalize(x)) <= raw["clip_range"] + 1e-9)
