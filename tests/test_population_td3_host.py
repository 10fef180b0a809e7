"""CPU (-m "not gpu"): a TD3 population's refusals (src/population.py TD3Population, csrc/agent_pop.inc gcrl_pop_create) name the
field and happen before any device work — so they are the same with and without a GPU.  Also the ABI entry that counts how a
population's launches were issued."""
import ctypes as C

import pytest

from oracle.agent_oracle import make_config


def _cfgs(P, **over):
    kw = dict(hidden_dim=64, layer_count=3, batch_size=64)
    kw.update(over)
    return [make_config("TD3", **kw) for _ in range(P)]


@pytest.mark.parametrize("P", [0, 17])
def test_member_count_refused(gcrl, P):
    with pytest.raises(gcrl._ffi.GcrlError, match="TD3Population: members"):
        gcrl.TD3Population(10, 3, _cfgs(P), 2, 8)


def test_shape_mismatch_refused(gcrl):
    cfgs = _cfgs(3)
    cfgs[2].batch_size = 128
    with pytest.raises(gcrl._ffi.GcrlError, match="batch_size"):
        gcrl.TD3Population(10, 3, cfgs, 2, 8)
    cfgs = _cfgs(2)
    cfgs[1].hidden_dim = 128
    with pytest.raises(gcrl._ffi.GcrlError, match="hidden_dim"):
        gcrl.TD3Population(10, 3, cfgs, 2, 8)
    cfgs = _cfgs(2)
    cfgs[1].ac_update_freq = 3
    with pytest.raises(gcrl._ffi.GcrlError, match="ac_update_freq"):
        gcrl.TD3Population(10, 3, cfgs, 2, 8)


@pytest.mark.parametrize("buffer_type", ["PER", "REPLAY"])
def test_non_her_buffer_refused(gcrl, buffer_type):
    cfgs = _cfgs(2)
    cfgs[1].buffer_type = buffer_type
    with pytest.raises(gcrl._ffi.GcrlError, match="buffer_type"):
        gcrl.TD3Population(10, 3, cfgs, 2, 8)


@pytest.mark.parametrize("B", [1024, 2048])
def test_large_batch_refused(gcrl, B):
    """B = 2048: the split dW form; B = 1024: the role-split critic phase — neither has a population form"""
    with pytest.raises(gcrl._ffi.GcrlError, match="batch_size"):
        gcrl.TD3Population(10, 3, _cfgs(2, batch_size=B), 2, 8)


def _native(gcrl, kinds, B=64):
    from gcrl_amd.src.agent import KIND, native_config
    out = []
    for k in kinds:
        c = make_config("TD3", hidden_dim=64, layer_count=3, batch_size=B)
        out.append(native_config(KIND[k], 10, 3, c, 8, num_critics=1 if k == "DDPG" else 2))
    return out


def _create(gcrl, native):
    arr = (gcrl._ffi.AgentConfig * len(native))(*native)
    p = gcrl._ffi.lib.gcrl_pop_create(arr, len(native))
    if p:
        gcrl._ffi.lib.gcrl_pop_destroy(p)
    return p, gcrl._ffi.last_error()


@pytest.mark.parametrize("kinds", [["TD3", "DDPG"], ["DDPG", "TD3"], ["TD3", "TD3", "SAC"]])
def test_engine_refuses_mixed_kinds(gcrl, kinds):
    p, msg = _create(gcrl, _native(gcrl, kinds))
    assert not p and "kind" in msg, msg


@pytest.mark.parametrize("kind", ["SAC", "TQC"])
def test_engine_refuses_sac_tqc(gcrl, kind):
    p, msg = _create(gcrl, _native(gcrl, [kind, kind]))
    assert not p and "kind" in msg, msg


@pytest.mark.parametrize("B", [1024, 2048, 4096])
def test_engine_refuses_td3_large_batch(gcrl, B):
    p, msg = _create(gcrl, _native(gcrl, ["TD3", "TD3"], B=B))
    assert not p and "batch_size" in msg, msg


def test_engine_refuses_td3_critic_count(gcrl):
    native = _native(gcrl, ["TD3", "TD3"])
    for n in native:
        n.num_critics = 1
    p, msg = _create(gcrl, native)
    assert not p and "num_critics" in msg, msg


def test_launch_counts_abi(gcrl):
    lib = gcrl._ffi.lib
    merged, alone = C.c_int64(-1), C.c_int64(-1)
    assert lib.gcrl_pop_launch_counts(None, C.byref(merged), C.byref(alone)) < 0
    assert "null" in gcrl._ffi.last_error()
    assert merged.value == -1 and alone.value == -1
    assert callable(gcrl.TD3Population.launch_counts) and callable(gcrl.DDPGPopulation.launch_counts)
    assert "TD3Population" in gcrl.__all__
