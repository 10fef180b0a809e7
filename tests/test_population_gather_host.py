"""No GPU: the host side of the population's merged replay gather and shared replay ring (src/population.py shared_ring /
merge_gather / gather_counts; include/gcrl.h gcrl_pop_set_gather_merge, gcrl_pop_gather_counts).  Every refusal names its field and
comes before any device work — this machine has no device to do any on."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest

from conftest import ROOT
from oracle.agent_oracle import make_config

ENTRIES = {"gcrl_pop_set_gather_merge": 2, "gcrl_pop_gather_counts": 4}     # name -> argument count


def _bare(gcrl, cls_name="DDPGPopulation", P=3, shared=True):
    """a population object with members that have configs and nothing else: any device work raises AttributeError"""
    cls = getattr(gcrl, cls_name)
    pop = object.__new__(cls)
    pop.shared_ring = shared
    pop.nenvs = 2
    pop.members = [SimpleNamespace(config=make_config(cls.AGENT.KIND_NAME, hidden_dim=64, layer_count=2, batch_size=64), _sac=False,
                                   obs_dim=10, ac_dim=3, num_critics=1) for _ in range(P)]
    return pop


@pytest.mark.parametrize("field,value", [("max_len", 5000), ("max_eps_len", 60), ("k_future", 2)])
def test_shared_ring_refuses_differing_ring_settings(gcrl, field, value):
    cfgs = [make_config("DDPG", hidden_dim=64, layer_count=2, batch_size=64) for _ in range(3)]
    assert getattr(cfgs[2], field) != value
    setattr(cfgs[2], field, value)
    with pytest.raises(gcrl._ffi.GcrlError, match=r"DDPGPopulation: %s: member 2 has" % field):
        gcrl.DDPGPopulation(10, 3, cfgs, 2, 8, shared_ring=True)


def test_shared_ring_refuses_copy_ring(gcrl):
    pop = _bare(gcrl)
    with pytest.raises(gcrl._ffi.GcrlError, match=r"DDPGPopulation: copy_ring: .*shared"):
        pop.exploit([(0, 1)], copy_ring=True)
    with pytest.raises(gcrl._ffi.GcrlError, match=r"TD3Population: copy_ring:"):
        _bare(gcrl, "TD3Population").exploit([(2, 0)], copy_ring=True)
    # the pairs are still judged first, and a population with its own rings gets past the refusal (to the device work: no handle here)
    with pytest.raises(gcrl._ffi.GcrlError, match=r"dst: member 7 of 3"):
        pop.exploit([(0, 7)], copy_ring=True)
    with pytest.raises(AttributeError):
        _bare(gcrl, shared=False).exploit([(0, 1)], copy_ring=True)


def test_shared_ring_refuses_save_and_load_state(gcrl, tmp_path):
    pop = _bare(gcrl)
    target = tmp_path / "state"
    with pytest.raises(gcrl._ffi.GcrlError, match=r"DDPGPopulation: shared_ring: save_state"):
        pop.save_state(str(target))
    assert not target.exists()                       # refused before anything was written
    with pytest.raises(gcrl._ffi.GcrlError, match=r"DDPGPopulation: shared_ring: load_state"):
        pop.load_state(str(target))


def test_shared_ring_refuses_more_envs_than_slots(gcrl):
    import numpy as np
    pop = _bare(gcrl)
    z = [None] * 3
    with pytest.raises(gcrl._ffi.GcrlError, match=r"DDPGPopulation: actions: member 1 steps 3 envs"):
        pop.process_step(z, [np.zeros((2, 3)), np.zeros((3, 3)), np.zeros((2, 3))], z, z, z)


def test_constructor_and_process_step_take_the_new_keywords(gcrl):
    import inspect
    sig = inspect.signature(gcrl.DDPGPopulation.__init__)
    assert sig.parameters["shared_ring"].default is False and sig.parameters["shared_ring"].kind is inspect.Parameter.KEYWORD_ONLY
    for cls in (gcrl.DDPG, gcrl.TD3Agent, gcrl.SACAgent, gcrl.TQCAgent):
        assert inspect.signature(cls.process_step).parameters["env0"].default == 0
    assert isinstance(gcrl.DDPGPopulation.merge_gather, property) and callable(gcrl.DDPGPopulation.gather_counts)


def test_new_entries_exist_in_header_ctypes_and_library(gcrl):
    header = open(os.path.join(ROOT, "include", "gcrl.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    so = C.CDLL(os.path.join(ROOT, "goal-conditioned-rl-framework_amd", "libgcrl_hip.so"))
    for e, nargs in ENTRIES.items():
        m = re.search(r"\bint %s\(([^)]*)\);" % e, header)
        assert m and len(m.group(1).split(",")) == nargs, e
        res, args = gcrl._ffi.PROTOTYPES[e]
        assert res is C.c_int and len(args) == nargs, e
        assert callable(getattr(gcrl._ffi.lib, e)) and getattr(so, e) is not None
    # null handles are argument errors, not crashes (no device involved)
    assert gcrl._ffi.lib.gcrl_pop_set_gather_merge(None, 1) < 0
    assert b"gcrl_pop_set_gather_merge" in gcrl._ffi.lib.gcrl_last_error()
    assert gcrl._ffi.lib.gcrl_pop_gather_counts(None, None, None, None) < 0
