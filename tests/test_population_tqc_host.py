"""CPU (-m "not gpu"): a TQC population's engine entry (include/gcrl.h gcrl_pop_create_layered, csrc/agent_pop.inc) and its Python
class (src/population.py TQCPopulation): the entry is declared, bound and exported, and every refusal names the field and happens
before any device work — so it is the same with and without a GPU.  (gcrl_pop_create / gcrl_pop_create_forms keep refusing TQC:
tests/test_population_sac_host.py and tests/test_population_td3_host.py pin that.  gcrl_pop_observe_act's refusal of a TQC population
needs a population, hence a device: tests/test_gpu_population_tqc.py.)"""
import ctypes as C
import os
import re

import pytest

from oracle.agent_oracle import make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "gcrl_pop_create_layered"


def _cfgs(P, kind="TQC", **over):
    kw = dict(hidden_dim=64, layer_count=3, batch_size=64)
    kw.update(over)
    return [make_config(kind, **kw) for _ in range(P)]


def _native(gcrl, kinds, num_critics=5, top_drop=2, n_quantiles=1, **over):
    from gcrl_amd.src.agent import KIND, native_config
    return [native_config(KIND[k], 10, 3, _cfgs(1, "SAC" if k in ("SAC", "TQC") else k, **over)[0], 8,
                          num_critics=num_critics if k == "TQC" else (1 if k == "DDPG" else 2), top_drop=top_drop if k == "TQC" else 0,
                          n_quantiles=n_quantiles if k == "TQC" else 1) for k in kinds]


def _create(gcrl, native, n=None):
    arr = (gcrl._ffi.AgentConfig * max(len(native), 1))(*native)
    p = getattr(gcrl._ffi.lib, ENTRY)(arr, len(native) if n is None else n)
    if p:
        gcrl._ffi.lib.gcrl_pop_destroy(p)
    return p, gcrl._ffi.last_error()


def test_entry_declared_bound_and_exported(gcrl):
    header = open(os.path.join(ROOT, "include", "gcrl.h")).read()
    assert re.search(r"gcrl_pop\*\s+%s\(const gcrl_agent_config\* cfgs, int32_t members\);" % ENTRY, header)
    assert ENTRY in gcrl._ffi.PROTOTYPES
    so = C.CDLL(os.path.join(ROOT, "goal-conditioned-rl-framework_amd", "libgcrl_hip.so"))
    assert getattr(so, ENTRY) is not None
    assert callable(getattr(gcrl._ffi.lib, ENTRY))
    assert "TQCPopulation" in gcrl.__all__
    assert gcrl.TQCPopulation.AGENT is gcrl.TQCAgent and gcrl.TQCPopulation.ENTRY == ENTRY
    assert gcrl.TQCPopulation.MERGE_ACTING_FROM == 17       # the merged acting launch is untimed for this kind: member by member by default


def test_null_array_and_member_count_refused(gcrl):
    p = getattr(gcrl._ffi.lib, ENTRY)(None, 2)
    assert not p and "%s: cfgs:" % ENTRY in gcrl._ffi.last_error(), gcrl._ffi.last_error()
    for P in (0, 17):
        p, msg = _create(gcrl, _native(gcrl, ["TQC"] * max(P, 1)), n=P)
        assert not p and "%s: members:" % ENTRY in msg, msg


@pytest.mark.parametrize("kinds", [["TQC", "SAC"], ["SAC", "TQC"], ["TQC", "TQC", "DDPG"]])
def test_mixed_kinds_refused(gcrl, kinds):
    p, msg = _create(gcrl, _native(gcrl, kinds))
    assert not p and "%s: kind:" % ENTRY in msg and "share" in msg, msg


@pytest.mark.parametrize("kind", ["SAC", "TD3", "DDPG"])
def test_other_kinds_are_pointed_at_their_entries(gcrl, kind):
    p, msg = _create(gcrl, _native(gcrl, [kind, kind]))
    assert not p and "%s: kind:" % ENTRY in msg and "gcrl_pop_create" in msg and "gcrl_pop_create_forms" in msg, msg


def test_distributional_variant_refused(gcrl):
    p, msg = _create(gcrl, _native(gcrl, ["TQC", "TQC"], n_quantiles=25))
    assert not p and "%s: n_quantiles:" % ENTRY in msg, msg


@pytest.mark.parametrize("nc", [1, 9])
def test_critic_count_refused(gcrl, nc):
    p, msg = _create(gcrl, _native(gcrl, ["TQC", "TQC"], num_critics=nc, top_drop=0))
    assert not p and "%s: num_critics:" % ENTRY in msg, msg
    with pytest.raises(gcrl._ffi.GcrlError, match="num_critics"):
        gcrl.TQCPopulation(10, 3, _cfgs(2, num_critics=nc, top_quantiles_to_drop=0), 2, 8)


def test_unequal_critic_counts_refused(gcrl):
    native = _native(gcrl, ["TQC", "TQC"])
    native[1].num_critics = 3
    p, msg = _create(gcrl, native)
    assert not p and "%s: num_critics:" % ENTRY in msg, msg
    cfgs = _cfgs(2)
    cfgs[1].num_critics = 3
    with pytest.raises(gcrl._ffi.GcrlError, match="TQCPopulation: num_critics"):
        gcrl.TQCPopulation(10, 3, cfgs, 2, 8)


def test_b1024_refused(gcrl):
    p, msg = _create(gcrl, _native(gcrl, ["TQC", "TQC"], batch_size=1024))
    assert not p and "%s: batch_size:" % ENTRY in msg, msg
    with pytest.raises(gcrl._ffi.GcrlError, match="batch_size"):
        gcrl.TQCPopulation(10, 3, _cfgs(2, batch_size=1024), 2, 8)


def test_h40_refused(gcrl):
    """the BatchNorm slab launches own 16 columns each"""
    p, msg = _create(gcrl, _native(gcrl, ["TQC", "TQC"], hidden_dim=40))
    assert not p and "%s: hidden_dim:" % ENTRY in msg, msg
    with pytest.raises(gcrl._ffi.GcrlError, match="hidden_dim"):
        gcrl.TQCPopulation(10, 3, _cfgs(2, hidden_dim=40), 2, 8)


def test_switched_off_slab_launches_refused(gcrl, monkeypatch):
    monkeypatch.setenv("GCRL_NO_BN_SLAB", "1")
    p, msg = _create(gcrl, _native(gcrl, ["TQC", "TQC"]))
    assert not p and "%s: GCRL_NO_BN_SLAB:" % ENTRY in msg, msg


def test_use_graph_2_refused(gcrl):
    native = _native(gcrl, ["TQC", "TQC"])
    for n in native:
        n.use_graph = 2
    p, msg = _create(gcrl, native)
    assert not p and "%s: use_graph:" % ENTRY in msg, msg


def test_shape_mismatch_refused(gcrl):
    native = _native(gcrl, ["TQC", "TQC"])
    native[1].hidden_dim = 128
    p, msg = _create(gcrl, native)
    assert not p and "%s: hidden_dim:" % ENTRY in msg, msg
    cfgs = _cfgs(2)
    cfgs[1].hidden_dim = 128
    with pytest.raises(gcrl._ffi.GcrlError, match="hidden_dim"):
        gcrl.TQCPopulation(10, 3, cfgs, 2, 8)


def test_python_side_refusals(gcrl):
    with pytest.raises(gcrl._ffi.GcrlError, match="TQCPopulation: buffer_type"):
        gcrl.TQCPopulation(10, 3, _cfgs(2, buffer_type="PER"), 2, 8)
    with pytest.raises(gcrl._ffi.GcrlError, match="TQCPopulation: members"):
        gcrl.TQCPopulation(10, 3, _cfgs(17), 2, 8)
    with pytest.raises(gcrl._ffi.GcrlError, match="TQCPopulation: members"):
        gcrl.TQCPopulation(10, 3, [], 2, 8)
