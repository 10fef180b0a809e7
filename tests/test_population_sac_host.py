"""CPU (-m "not gpu"): a SAC population's refusals (src/population.py SACPopulation, csrc/agent_pop.inc gcrl_pop_create) name the
field and happen before any device work — so they are the same with and without a GPU.  SAC populations are created through
gcrl_pop_create_forms (gcrl_pop_create keeps refusing SAC naming kind: tests/test_population_td3_host.py pins that).  Also the ABI
entries that report the population's launch forms.  (gcrl_pop_observe_act's refusal of a SAC population needs a population, hence a device:
tests/test_gpu_population_sac.py test_engine_refuses_merged_acting.)"""
import pytest

from oracle.agent_oracle import make_config


def _cfgs(P, kind="SAC", **over):
    kw = dict(hidden_dim=64, layer_count=3, batch_size=64)
    kw.update(over)
    return [make_config(kind, **kw) for _ in range(P)]


def _native(gcrl, kinds, **over):
    from gcrl_amd.src.agent import KIND, native_config
    return [native_config(KIND[k], 10, 3, _cfgs(1, "SAC" if k in ("SAC", "TQC") else k, **over)[0], 8, num_critics=1 if k == "DDPG" else 2) for k in kinds]


def _create(gcrl, native, entry="gcrl_pop_create_forms"):
    arr = (gcrl._ffi.AgentConfig * len(native))(*native)
    p = getattr(gcrl._ffi.lib, entry)(arr, len(native))
    if p:
        gcrl._ffi.lib.gcrl_pop_destroy(p)
    return p, gcrl._ffi.last_error()


def test_engine_refuses_tqc(gcrl):
    p, msg = _create(gcrl, _native(gcrl, ["TQC", "TQC"]))
    assert not p and "kind" in msg and "TQC populations are not implemented" in msg, msg


def test_engine_refuses_b1024(gcrl):
    p, msg = _create(gcrl, _native(gcrl, ["SAC", "SAC"], batch_size=1024))
    assert not p and "gcrl_pop_create: batch_size:" in msg, msg
    with pytest.raises(gcrl._ffi.GcrlError, match="batch_size"):
        gcrl.SACPopulation(10, 3, _cfgs(2, batch_size=1024), 2, 8)


def test_engine_refuses_h40(gcrl):
    """40 % 4 == 0 passes the row-chain rule; the BatchNorm slab launches own 16 columns each"""
    p, msg = _create(gcrl, _native(gcrl, ["SAC", "SAC"], hidden_dim=40))
    assert not p and "gcrl_pop_create: hidden_dim:" in msg, msg
    with pytest.raises(gcrl._ffi.GcrlError, match="hidden_dim"):
        gcrl.SACPopulation(10, 3, _cfgs(2, hidden_dim=40), 2, 8)


@pytest.mark.parametrize("kinds", [["SAC", "TD3"], ["TD3", "SAC"], ["SAC", "SAC", "DDPG"], ["SAC", "TQC"]])
def test_engine_refuses_mixed_kinds(gcrl, kinds):
    p, msg = _create(gcrl, _native(gcrl, kinds))
    assert not p and "gcrl_pop_create: kind:" in msg, msg


def test_engine_refuses_layer_per_launch_path(gcrl):
    native = _native(gcrl, ["SAC", "SAC"])
    for n in native:
        n.pipeline_steps = 0
    p, msg = _create(gcrl, native)
    assert not p and "gcrl_pop_create: pipeline_steps:" in msg, msg


def test_engine_refuses_critic_count(gcrl):
    native = _native(gcrl, ["SAC", "SAC"])
    for n in native:
        n.num_critics = 1
    p, msg = _create(gcrl, native)
    assert not p and "gcrl_pop_create: num_critics:" in msg, msg


@pytest.mark.parametrize("knob", ["GCRL_NO_BN_SLAB", "GCRL_NO_SPLIT_ROLES", "GCRL_NO_HEADS_FOLD"])
def test_engine_refuses_switched_off_path(gcrl, monkeypatch, knob):
    monkeypatch.setenv(knob, "1")
    p, msg = _create(gcrl, _native(gcrl, ["SAC", "SAC"]))
    assert not p and ("gcrl_pop_create: %s:" % knob) in msg, msg


@pytest.mark.parametrize("P", [0, 17])
def test_member_count_refused(gcrl, P):
    with pytest.raises(gcrl._ffi.GcrlError, match="SACPopulation: members"):
        gcrl.SACPopulation(10, 3, _cfgs(P), 2, 8)
    if P:
        p, msg = _create(gcrl, _native(gcrl, ["SAC"] * P))
        assert not p and "gcrl_pop_create: members:" in msg, msg


def test_shape_mismatch_refused(gcrl):
    cfgs = _cfgs(2)
    cfgs[1].hidden_dim = 128
    with pytest.raises(gcrl._ffi.GcrlError, match="hidden_dim"):
        gcrl.SACPopulation(10, 3, cfgs, 2, 8)
    native = _native(gcrl, ["SAC", "SAC"])
    native[1].hidden_dim = 128
    p, msg = _create(gcrl, native)
    assert not p and "gcrl_pop_create: hidden_dim:" in msg, msg


def test_forms_abi(gcrl):
    lib = gcrl._ffi.lib
    assert lib.gcrl_pop_forms(None) < 0
    assert "null" in gcrl._ffi.last_error()
    import ctypes as C
    want, cap = (C.c_int64 * 3)(-1, -1, -1), (C.c_int64 * 3)(-1, -1, -1)
    assert lib.gcrl_pop_forms_terms(None, want, cap) < 0 and "null" in gcrl._ffi.last_error()
    assert list(want) == [-1, -1, -1] and list(cap) == [-1, -1, -1]
    assert callable(gcrl.SACPopulation.forms_terms)
    assert callable(gcrl.SACPopulation.forms) and callable(gcrl.TD3Population.forms)
    assert "SACPopulation" in gcrl.__all__
    assert gcrl.SACPopulation.AGENT is gcrl.SACAgent and gcrl.SACPopulation.NUM_CRITICS == 2
