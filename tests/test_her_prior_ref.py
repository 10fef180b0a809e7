"""Host tests (no GPU) of tests/her_prior_ref.py, the numpy definition of prior-data replay (prior_buffer= / prior_rows=;
csrc/her_prior.hip): the restatement's own properties, every keyword refusal that precedes device work on the four agents and the
four populations, the ABI entries, and the new unit's kernel metadata."""
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT
from oracle.agent_oracle import make_config

import her_prior_ref as PR

F32 = np.float32


def bits(x):
    return np.ascontiguousarray(np.asarray(x, F32)).view(np.uint32)


def _gather(gen, rows, S, A, spa=True):
    """a gather_update result of `rows` rows as the engine's matrices, every float distinct; spa pre-filled with NaN behind S4"""
    ldx, S4 = (S + A + 3) // 4 * 4, (S + 3) // 4 * 4
    sa = gen.standard_normal((rows, ldx)).astype(F32)
    nsa = gen.standard_normal((rows, ldx)).astype(F32)     # (columns behind S4: whatever a partial wave left)
    sp = np.full((rows, ldx), np.nan, F32)
    sp[:, :S4] = sa[:, :S4]
    return sa, nsa, (sp if spa else None), gen.standard_normal(rows).astype(F32), gen.integers(0, 2, rows).astype(F32)


# ---------------------------------------------------------------- 1. the restatement's own properties
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("B,Bd", [(64, 1), (64, 20), (64, 63), (5, 4), (2, 1)])
@pytest.mark.parametrize("dims", [(10, 3), (23, 4), (70, 4)])
def test_head_rows_untouched_and_tail_is_the_prior_batches(dims, B, Bd, M):
    S, A = dims
    S4 = (S + 3) // 4 * 4
    gen = np.random.default_rng(B * 131 + Bd * 7 + M)
    main, prior = _gather(gen, M * B, S, A), _gather(gen, M * Bd, S, A)
    keep = tuple(None if x is None else x.copy() for x in main)
    out = PR.mix(main, prior, B, Bd, M, S)
    for x, y in zip(main, keep):                                  # the inputs are left alone
        assert np.array_equal(bits(x), bits(y))
    for j in range(M):
        head, tail = slice(j * B, j * B + B - Bd), slice(j * B + B - Bd, (j + 1) * B)
        pj = slice(j * Bd, (j + 1) * Bd)
        for k in range(5):
            assert np.array_equal(bits(out[k][head]), bits(main[k][head])), (j, k)
        assert np.array_equal(bits(out[0][tail]), bits(prior[0][pj]))
        assert np.array_equal(bits(out[1][tail][:, :S4]), bits(prior[1][pj][:, :S4])) and not out[1][tail][:, S4:].any()
        assert np.array_equal(bits(out[2][tail][:, :S4]), bits(prior[2][pj][:, :S4])) and np.isnan(out[2][tail][:, S4:]).all()
        assert np.array_equal(bits(out[3][tail]), bits(prior[3][pj])) and np.array_equal(bits(out[4][tail]), bits(prior[4][pj]))
    assert np.isnan(out[2][:, S4:]).all()                          # spa's columns behind S4 are nobody's to write


def test_mapping_covers_the_tail_rows_once_and_nothing_else():
    for B, Bd, nb in ((64, 1, 3), (64, 63, 2), (256, 128, 4), (7, 3, 5)):
        seen = {}
        for t in range(nb * Bd):
            slot, row = PR.slot_row(B, Bd, t)
            assert 0 <= slot < nb and B - Bd <= row < B
            seen[(slot, row)] = seen.get((slot, row), 0) + 1
        assert len(seen) == nb * Bd and set(seen.values()) == {1}
    assert PR.counters_after(100, 9, 6, 20) == (220, 15) and PR.counters_after(100, 9, 6, 20, sample_mode=False) == (100, 15)
    assert PR.rows_ok(64, 1) and PR.rows_ok(64, 63) and not PR.rows_ok(64, 64) and not PR.rows_ok(64, 0) and not PR.rows_ok(1, 1)
    assert not PR.rows_ok(64, True) and not PR.rows_ok(64, 2.0)
    with pytest.raises(AssertionError):
        PR.mix(_gather(np.random.default_rng(0), 4, 10, 3), _gather(np.random.default_rng(1), 4, 10, 3), 4, 4, 1, 10)


# ---------------------------------------------------------------- 2. keyword refusals before any device work
def _stub(HERBuffer, rng="device", prioritise=None, normalize="push", flags=(True, False)):
    """a prior ring as its constructor leaves it, without the device its last lines ask for"""
    b = HERBuffer.__new__(HERBuffer)
    b.rng, b.prioritise, b.normalize, b._h = SimpleNamespace(mode=rng), prioritise, normalize, None
    b.obs_normalize, b.g_normalize = flags
    return b


def test_python_refusals_name_prior_buffer_or_prior_rows(gcrl):
    err = gcrl._ffi.GcrlError
    from gcrl_amd.src.buffer import HERBuffer, _check_prior
    good = _stub(HERBuffer)
    assert _check_prior("x", None, None, 64) == 0 and _check_prior("x", good, 20, 64) == 20 and _check_prior("x", good, np.int64(63), 64) == 63
    kw = dict(hidden_dim=64, layer_count=3, batch_size=64)
    for name, cls, pop in (("DDPG", gcrl.DDPG, gcrl.DDPGPopulation), ("TD3", gcrl.TD3Agent, gcrl.TD3Population),
                           ("SAC", gcrl.SACAgent, gcrl.SACPopulation), ("TQC", gcrl.TQCAgent, gcrl.TQCPopulation)):
        cfg = make_config(name, **kw)
        agent = lambda c=cfg, **k: cls(10, 3, c, None, 2, 4, **k)
        members = lambda c=None, **k: pop(10, 3, c or [make_config(name, **kw) for _ in range(2)], 2, 4, **k)
        for who, build in ((cls.__name__, agent), (pop.__name__, members)):
            with pytest.raises(err, match=f"{who}: prior_rows"):                      # exactly one of the two keywords
                build(prior_buffer=good)
            with pytest.raises(err, match=f"{who}: prior_buffer"):
                build(prior_rows=20)
            for bad in (0, 64, 65, -1, 2.5, True, "20"):                               # 1 <= Bd <= B - 1, an integer
                with pytest.raises(err, match=f"{who}: prior_rows"):
                    build(prior_buffer=good, prior_rows=bad)
            with pytest.raises(err, match=f"{who}: prior_buffer"):                    # not a HERBuffer
                build(prior_buffer=object(), prior_rows=20)
            for mode in ("python", "engine"):                                          # rng is not "device"
                with pytest.raises(err, match=f"{who}: prior_buffer.*rng"):
                    build(prior_buffer=_stub(HERBuffer, rng=mode), prior_rows=20)
            with pytest.raises(err, match=f"{who}: prior_buffer.*tree"):              # the prior ring carries a tree
                build(prior_buffer=_stub(HERBuffer, prioritise="energy"), prior_rows=20)
            with pytest.raises(err, match=f"{who}: prior_buffer.*normalize"):         # normalize modes differ, both ways
                build(prior_buffer=_stub(HERBuffer, normalize="sample"), prior_rows=20)
            with pytest.raises(err, match=f"{who}: prior_buffer.*normalize"):
                build(prior_buffer=good, prior_rows=20, normalize="sample")
        with pytest.raises(err, match=f"{cls.__name__}: prior_buffer"):                # normalize="sample" with other flags than the agent's
            agent(prior_buffer=_stub(HERBuffer, normalize="sample", flags=(True, True)), prior_rows=20, normalize="sample")
        for bt in ("PER", "REPLAY"):                                                   # the main buffer_type is not "HER"
            c2 = make_config(name, **kw)
            c2.buffer_type = bt
            with pytest.raises(err, match=f"{cls.__name__}: prior_buffer"):
                agent(c2, prior_buffer=good, prior_rows=20)
            with pytest.raises(err, match=f"{pop.__name__}: prior_buffer"):
                members([c2, make_config(name, **kw)], prior_buffer=good, prior_rows=20)
        with pytest.raises(err, match=f"{pop.__name__}: prior_buffer"):                # a list of rings: one per member
            members(prior_buffer=[good], prior_rows=20)
        with pytest.raises(err, match=f"{pop.__name__}: prior_buffer.*rng"):           # ... each held to the same rules
            members(prior_buffer=[good, _stub(HERBuffer, rng="engine")], prior_rows=20)
    with pytest.raises(err, match="gather_update_mixed: prior_rows"):
        HERBuffer.gather_update_mixed(good, good, 64, 64)
    from gcrl_amd.src.dp import DataParallelUpdater                                    # the agent is under a gradient exchange
    with pytest.raises(err, match="prior_buffer"):
        DataParallelUpdater(SimpleNamespace(per_draw="host", prior_buffer=good))


def test_abi_declares_the_new_entries(gcrl):
    lib = gcrl._ffi.lib
    names = ("gcrl_agent_set_prior", "gcrl_agent_get_prior", "gcrl_agent_prior_counts", "gcrl_agent_read_batch", "gcrl_her_gather_update_mixed")
    hdr = open(os.path.join(ROOT, "include", "gcrl.h")).read()
    for name in names:
        assert hasattr(lib, name) and name in hdr and name in gcrl._ffi.PROTOTYPES, name
    # null handles: refused by name, no device touched
    assert lib.gcrl_agent_set_prior(None, None, 0) == -1 and b"gcrl_agent_set_prior" in lib.gcrl_last_error()
    assert lib.gcrl_agent_prior_counts(None, None, None) == -1 and b"gcrl_agent_prior_counts" in lib.gcrl_last_error()
    assert lib.gcrl_agent_read_batch(None, 0, None, None, None, None) == -1 and b"gcrl_agent_read_batch" in lib.gcrl_last_error()
    assert lib.gcrl_her_gather_update_mixed(None, None, 64, 20, 1, None, None, None, 16, None, None, None) == -1
    assert b"gcrl_her_gather_update_mixed" in lib.gcrl_last_error()


def test_shared_prior_ring_needs_shared_normalisers(gcrl):
    """populations, normalize="sample": members that share a prior ring must share the normaliser objects their flags need"""
    from gcrl_amd.src.population import check_shared_prior_normalizers as check
    err = gcrl._ffi.GcrlError
    ring, other, z0, z1, g0 = object(), object(), object(), object(), object()

    def member(pb, zo, zg=None, normalize="sample", flags=(True, False)):
        return SimpleNamespace(prior_buffer=pb, normalize=normalize, obs_normalize=flags[0], g_normalize=flags[1],
                               buffer=SimpleNamespace(obs_normalizer=zo, dg_normalizer=zg))
    check("P", [member(ring, z0), member(ring, z0)])                                   # shared ring, shared normaliser
    check("P", [member(ring, z0), member(other, z1)])                                  # one prior ring per member
    check("P", [member(ring, z0, normalize="push"), member(ring, z1, normalize="push")])   # nothing is normalised at gather time
    check("P", [member(None, z0), member(None, z1)])
    check("P", [member(ring, z0, g0), member(ring, z0, object())])                     # g_normalize off: the goal normaliser is not used
    with pytest.raises(err, match="P: prior_buffer: members 0 and 1"):
        check("P", [member(ring, z0), member(ring, z1)])
    with pytest.raises(err, match="P: prior_buffer: members 0 and 2"):
        check("P", [member(ring, z0), member(other, z1), member(ring, None)])
    with pytest.raises(err, match="P: prior_buffer"):
        check("P", [member(ring, z0, g0, flags=(True, True)), member(ring, z0, object(), flags=(True, True))])


def test_new_kernel_uses_no_scratch_no_lds_and_does_not_spill(tmp_path):
    """her_prior.hip compiled to gfx950 assembly with the Makefile's flags: by the kernel's metadata 0 bytes of scratch, no spills
    and no LDS (the register figures of one compiler build are in profiles/r25_prior_unchanged_path.txt and DESIGN.md §4n)"""
    csrc = os.path.join(ROOT, "goal-conditioned-rl-framework_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)).split()
    hipcc = os.environ.get("HIPCC", re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M).group(1))
    assert "her_prior.hip" in re.search(r"^SRCS\s*=\s*(.*)$", mk, re.M).group(1).split() and "-ffp-contract=off" in flags and "-O3" in flags
    asm = tmp_path / "her_prior.s"
    subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(csrc, "her_prior.hip"), "-o", str(asm)], check=True, cwd=csrc)
    seen = []
    for blk in re.split(r"\n\s+- \.agpr_count:", asm.read_text())[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        field = lambda f: int(re.search(rf"\.{f}:\s+(\d+)", blk).group(1))
        seen.append(name)
        assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0, name
        assert field("group_segment_fixed_size") == 0, name
    assert len(seen) == 1 and "her_place_rows_kernel" in seen[0], seen
