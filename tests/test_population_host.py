"""CPU (-m "not gpu"): a DDPG population's refusals (src/population.py, csrc/agent_pop.inc gcrl_pop_create) name the field and
happen before any device work — so they are the same with and without a GPU."""
import ctypes as C

import pytest

from oracle.agent_oracle import make_config


def _cfgs(P, **over):
    return [make_config("DDPG", hidden_dim=64, layer_count=3, batch_size=64, **over) for _ in range(P)]


@pytest.mark.parametrize("P", [0, 17])
def test_member_count_refused(gcrl, P):
    with pytest.raises(gcrl._ffi.GcrlError, match="members"):
        gcrl.DDPGPopulation(10, 3, _cfgs(P), 2, 8)


def test_shape_mismatch_refused(gcrl):
    cfgs = _cfgs(3)
    cfgs[2].batch_size = 128
    with pytest.raises(gcrl._ffi.GcrlError, match="batch_size"):
        gcrl.DDPGPopulation(10, 3, cfgs, 2, 8)
    cfgs = _cfgs(2)
    cfgs[1].hidden_dim = 128
    with pytest.raises(gcrl._ffi.GcrlError, match="hidden_dim"):
        gcrl.DDPGPopulation(10, 3, cfgs, 2, 8)


@pytest.mark.parametrize("buffer_type", ["PER", "REPLAY"])
def test_non_her_buffer_refused(gcrl, buffer_type):
    cfgs = _cfgs(2)
    cfgs[1].buffer_type = buffer_type
    with pytest.raises(gcrl._ffi.GcrlError, match="buffer_type"):
        gcrl.DDPGPopulation(10, 3, cfgs, 2, 8)


def _native(gcrl, cfgs, **over):
    from gcrl_amd.src.agent import KIND, native_config
    out = [native_config(KIND["DDPG"], 10, 3, c, 8) for c in cfgs]
    for k, v in over.items():
        i, field = k.split("_", 1)
        setattr(out[int(i[1:])], field, v)
    return out


def _create(gcrl, native):
    arr = (gcrl._ffi.AgentConfig * len(native))(*native)
    p = gcrl._ffi.lib.gcrl_pop_create(arr, len(native))
    if p:
        gcrl._ffi.lib.gcrl_pop_destroy(p)
    return p, gcrl._ffi.last_error()


@pytest.mark.parametrize("kind", [1, 2, 3])   # TD3, SAC, TQC
def test_engine_refuses_other_kinds(gcrl, kind):
    p, msg = _create(gcrl, _native(gcrl, _cfgs(2), m1_kind=kind))
    assert not p and "kind" in msg, msg


@pytest.mark.parametrize("field,value", [("obs_dim", 11), ("batch_size", 32), ("layer_count", 2), ("gradient_step", 4),
                                         ("ac_update_freq", 2), ("use_graph", 0), ("device", 1)])
def test_engine_refuses_mismatched_shared_fields(gcrl, field, value):
    p, msg = _create(gcrl, _native(gcrl, _cfgs(2), **{"m1_" + field: value}))
    assert not p and field in msg, msg


def test_engine_refuses_non_rowchain_configs(gcrl):
    p, msg = _create(gcrl, _native(gcrl, _cfgs(2), m0_pipeline_steps=0, m1_pipeline_steps=0))
    assert not p and "pipeline_steps" in msg, msg
    cfgs = [make_config("DDPG", hidden_dim=66, layer_count=3, batch_size=64) for _ in range(2)]
    p, msg = _create(gcrl, _native(gcrl, cfgs))
    assert not p and "hidden_dim" in msg, msg


def test_engine_refuses_member_counts(gcrl):
    native = _native(gcrl, _cfgs(1))
    arr = (gcrl._ffi.AgentConfig * 1)(*native)
    for P in (0, 17, -1):
        assert not gcrl._ffi.lib.gcrl_pop_create(arr, P)
        assert "members" in gcrl._ffi.last_error()
    assert gcrl._ffi.lib.gcrl_pop_size(None) == -1
    out = C.c_void_p()
    assert gcrl._ffi.lib.gcrl_pop_member(None, 0, C.byref(out)) < 0
