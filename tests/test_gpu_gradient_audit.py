"""GPU (-m gpu): every launch form of the update step audited PER ELEMENT against tests/grad_ref.py — torch autograd on the CPU, in
fp32 and fp64 on the same fp32 inputs — at the shapes where a launch rule of gcrl_agent_create switches.  The other half of
tests/test_gpu_optimiser_audit.py, which takes the gradient as given.

Each case (tests/grad_cases.py: the table, the inputs, the bound) is one `update(step)` from parameters set through the views, with
an explicit batch, injected noise and, where the case says so, importance weights through `UpdateInputs.weights_host`.  After the
step `grad:<net>` of every net that stepped, `grad:log_alpha`, the tuple, `bn_running_mean` / `bn_running_var` and, on the
layer-per-launch schedule, `td_abs` and the pi(s) columns of `batch_spa` (the row chain writes neither: td_abs has one consumer,
prioritised replay, which runs pipeline=0; pi(s) stays inside the chain launches, and an error in it shows in the actor's gradient)
are read and held to

    max |hip - ref64|  <=  max(K_REF * e32, RTOL * scale)          (tests/fullsize.py's K_REF and RTOL)

per quantity and per parameter tensor (grad_cases.judge).  The actor phase of the reference runs through the critics the ENGINE
stepped, read back: an optimiser ulp is not charged to the gradient.  Units near an activation kink are listed from the reference's
own values and their flip vectors fitted (fullsize.explain_flips); a deviation that needs an unlisted unit fails the case.

The form is asserted, never assumed: Agent.update_forms() (rows per workgroup, row chain, split_roles, rc_merge, split_k,
rc_merge_k, ddpg_ksplit, opt_fuse, bn_slab, bn_rsplit), meetings() and rowchain_form() against what the case is there for; a form
the device refuses because it is shared skips the case with that reason.  Switches read at agent creation are set with monkeypatch
before the agent is built; the three switches read once per process (GCRL_NO_TG_FOLD, GCRL_NO_HEADS_FOLD, GCRL_SLAB_MEET) run in
one child process each, which prints what it read as JSON; the parent applies the bound.

Every case prints its forms, its coverage counts (on the fp64 reference's values; a claimed count of zero fails) and err / bound
per quantity; test_records/gradient_audit.json is rewritten after every case.

Not audited here: `update_many` and the population launches.  They are held BITWISE to what is audited here —
test_gpu_parity.py::test_update_many_equals_repeated_update and ::test_pipelined_ddpg_is_bitwise_the_sequential_path (update_many
against repeated update()), test_gpu_population.py / test_gpu_population_td3.py / test_gpu_population_sac.py /
test_gpu_population_tqc.py (every member against the standalone agent running the same forms).  The distributional TQC variant has
its own pins (test_gpu_quantile_kernels.py).
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import grad_cases as gc
from oracle.agent_oracle import make_config

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
WAITING = {"ddpg_ksplit": 1, "opt_fuse": 1, "rc_merge": 1, "rc_merge_k": 1, "bn_rsplit": 4}     # forms a shared device refuses: their "on" value
RECORD = dict(cases={}, worst={})


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _table():
    """The table for this device where there is one (the two-role boundary follows its CUs), the MI355X's otherwise (collection
    without a GPU)."""
    try:
        return gc.table(_cus() if torch.cuda.is_available() else gc.MI355X_CUS)
    except Exception:
        return gc.table()


TABLE = _table()


# ------------------------------------------------------------------------------------------------------------------ one case on the device
def run_on_device(gcrl, case, setenv=None):
    """Builds the agent, runs the one update, -> dict of plain lists (JSON-able): forms, meetings, rowchain_form, grads, quantities,
    the stepped critics.  setenv(name, value | None): how creation switches are set (monkeypatch in the parent, os.environ in a child)."""
    _ffi, lib = gcrl._ffi, gcrl._ffi.lib
    for sw in gc.CREATION_SWITCHES:
        setenv(sw, "1" if sw in case.env else None)
    inp = gc.inputs(case)
    cfg = make_config(case.kind, **gc.config_overrides(case))
    cls = dict(DDPG=gcrl.DDPG, TD3=gcrl.TD3Agent, SAC=gcrl.SACAgent, TQC=gcrl.TQCAgent)[case.kind]
    kw = dict(pipeline=0) if case.pipeline == 0 else {}
    ag = cls(case.S, case.A, cfg, None, nenvs=1, gradient_step=2, rng="engine", seed=7, **kw)
    for name, vec in inp.nets.items():
        ag.actor._set(name, vec)
    if case.kind in ("SAC", "TQC"):
        ag.actor._set("log_alpha", np.array([inp.log_alpha], F32))
    forms = ag.update_forms()
    dev = lambda x: torch.from_numpy(x).cuda()
    extra = {k: dev(getattr(inp, k)) for k in ("noise", "eps_next", "eps_cur") if getattr(inp, k) is not None}
    batch = tuple(dev(x) for x in inp.batch)
    if inp.weights is None:
        tup = [float(x) for x in ag.update(case.step, batch=batch, **extra)]
    else:
        ag.set_train()
        ins, keep = ag._inject(batch, extra.get("noise"), extra.get("eps_next"), extra.get("eps_cur"))
        w = np.ascontiguousarray(inp.weights, dtype=F32)
        ins.weights_host = w.ctypes.data
        ticket = C.c_int64(-1)
        n = _ffi.check(lib.gcrl_agent_update(ag._h, None, int(case.step), C.byref(ins), C.byref(ticket), _ffi.stream_handle()))
        tup = [float(x) for x in ag._metrics(ticket.value, n)]
        del keep
    get = ag.actor._get
    C_ = len(ag.critics)
    out = dict(id=case.id, forms=forms, forms_after=ag.update_forms(), meetings=int(ag.meetings()), rowchain_form=int(ag.rowchain_form()),
               grads={f"critic_{i}": get(f"grad:critic_{i}").tolist() for i in range(C_)},
               critics_after=[get(f"critic_{i}").tolist() for i in range(C_)], q={})
    if not forms["rowchain"]:
        out["q"]["td_abs"] = get("td_abs").tolist()
    for j, v in enumerate(tup):
        out["q"][f"tuple[{j}]"] = [v]
    if inp.actor_step:
        out["grads"]["actor"] = get("grad:actor").tolist()
        if not forms["rowchain"]:
            ldx = (case.S + case.A + 3) // 4 * 4
            spa = get("batch_spa")[: case.B * ldx].reshape(case.B, ldx)
            out["q"]["pi"] = spa[:, case.S:case.S + case.A].reshape(-1).tolist()
            out["spa_state_exact"] = bool(np.array_equal(spa[:, :case.S], inp.batch[0]))
    if case.kind in ("SAC", "TQC"):
        if inp.alpha_step:
            out["q"]["grad:log_alpha"] = get("grad:log_alpha").tolist()
        out["q"]["bn_running_mean"] = get("bn_running_mean").tolist()
        out["q"]["bn_running_var"] = get("bn_running_var").tolist()
    return out


def covers(claims, counts):
    print("  covers " + " ".join(f"{k}={int(v)}" for k, v in counts.items()) + f"  (claims {sorted(claims)})")
    zero = [k for k in claims if int(counts.get(k, 0)) == 0]
    assert not zero, f"the case misses {zero}"


def check_forms(case, got):
    """The form the case is there for, against what the handle reports.  Skips where a form with waits between workgroups is refused."""
    forms = got["forms"]
    print(f"  {case.id}: {case.why}\n  forms {forms}  meetings {got['meetings']}  rowchain_form {got['rowchain_form']}")
    assert got["forms_after"] == forms, ("a launch form changed during the step", forms, got["forms_after"])
    for key, want in case.expect.items():
        if forms[key] != want and WAITING.get(key) == want:
            pytest.skip(f"{case.id}: {key} is not admissible on this device (shared GPU, or too few CUs for its workgroups): the rule boundary "
                        f"this case is there for stays unaudited")
        assert forms[key] == want, (case.id, key, forms[key], want)
    m = got["meetings"]
    assert bool(m & 8) == bool(forms["opt_fuse"]) and bool(m & 1) == (forms["bn_rsplit"] > 1), (m, forms)
    assert bool(m & 2) == bool(forms["rc_merge"] or forms["rc_merge_k"] or forms["ddpg_ksplit"]), (m, forms)
    if case.kind == "DDPG" and forms["rowchain"]:
        if "GCRL_RC_GLOBAL_MUL" in case.env or case.L < 2:
            assert got["rowchain_form"] == 0, got["rowchain_form"]
        else:
            assert got["rowchain_form"] != 0, "the default agent does not report the LDS-multiplier form"
    if not forms["rowchain"] or case.kind in ("SAC", "TQC"):
        assert got["rowchain_form"] == 0


def _record(case, got, ref, rows, fitted):
    worst = max(r["ratio"] for r in rows)
    form = "rowchain" if got["forms"]["rowchain"] else "layer_per_launch"
    key = f"{case.kind}/{form}"
    RECORD["worst"][key] = max(RECORD["worst"].get(key, 0.0), worst)
    RECORD["cases"][case.id] = dict(why=case.why, forms=got["forms"], meetings=got["meetings"], rowchain_form=got["rowchain_form"],
                                    kink_units_listed=[list(u) for u in ref.units], kink_units_fitted=fitted, covers=ref.cover,
                                    worst_err_over_bound=worst,
                                    quantities={r["quantity"]: dict(err_over_bound=r["ratio"], e32=r["e32"], scale=r["scale"]) for r in rows})
    os.makedirs(os.path.join(ROOT, "test_records"), exist_ok=True)
    with open(os.path.join(ROOT, "test_records", "gradient_audit.json"), "w") as f:
        json.dump(dict(note="per-element gradients, td_abs, pi(s), the tuple and BatchNorm's running statistics of one update() per launch form "
                            "against tests/grad_ref.py (torch autograd, fp64): err / bound per quantity (<= 1 passes), bound = max(K_REF * e32, "
                            "RTOL * scale) (tests/grad_cases.py)", worst_err_over_bound=RECORD["worst"],
                       kink_units=dict(listed=sum(len(c["kink_units_listed"]) for c in RECORD["cases"].values()),
                                       fitted=sum(c["kink_units_fitted"] for c in RECORD["cases"].values())),
                       cases=RECORD["cases"]), f, indent=1, sort_keys=True)


def audit(case, got):
    check_forms(case, got)
    inp = gc.inputs(case)
    ref = gc.references(case, inp, critics_after=[np.asarray(v, F32) for v in got["critics_after"]])
    covers(case.claims, ref.cover)
    print(f"  near a kink: {len(ref.units)} units listed {ref.units}")
    if "spa_state_exact" in got:
        assert got["spa_state_exact"], "the state columns of batch_spa are not the batch's"
    dev = dict(grads={n: np.asarray(v, F32) for n, v in got["grads"].items()}, **{k: np.asarray(v, np.float64) for k, v in got["q"].items()})
    want = set(gc.quantities(ref.step, ref.r64)) - ({"td_abs", "pi"} if got["forms"]["rowchain"] else set())
    assert set(got["q"]) == want, (sorted(got["q"]), sorted(want))
    rows, fitted = gc.judge(case, ref, dev)
    _record(case, got, ref, rows, fitted)
    worst = max(rows, key=lambda r: r["ratio"])
    print(f"  {case.id}: worst err/bound {worst['ratio']:.3f} ({worst['quantity']}) over {len(rows)} quantities; kink flips fitted {fitted} of "
          f"{len(ref.units)} listed")
    bad = [(r["quantity"], r["err"], r["e32"], r["scale"], round(r["ratio"], 3)) for r in rows if not r["ok"]]
    assert not bad, (case.id, bad[:12])


# ------------------------------------------------------------------------------------------------------------------ in this process
@pytest.fixture(autouse=True)
def _reference_on_one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("case", [c for c in TABLE if not c.proc], ids=lambda c: c.id)
def test_update_gradients_against_the_fp64_reference(gcrl, monkeypatch, case):
    for sw in gc.PROCESS_SWITCHES:
        assert sw not in os.environ, f"{sw} is read once per process: unset it for this file"

    def setenv(name, value):
        monkeypatch.delenv(name, raising=False) if value is None else monkeypatch.setenv(name, value)

    audit(case, run_on_device(gcrl, case, setenv))


# ------------------------------------------------------------------------------------------------------------------ child processes
CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import gcrl_amd as gcrl
import test_gpu_gradient_audit as T

def setenv(name, value):
    os.environ.pop(name, None) if value is None else os.environ.__setitem__(name, value)

cases = T.gc.by_id(int(sys.argv[2]))
for cid in sys.argv[3:]:
    print("RESULT " + json.dumps(T.run_on_device(gcrl, cases[cid], setenv)), flush=True)
"""


@pytest.mark.parametrize("switch", gc.PROCESS_SWITCHES)
def test_update_gradients_under_a_once_per_process_switch(switch):
    """GCRL_NO_TG_FOLD (the sampling backward in its own launch), GCRL_NO_HEADS_FOLD (the heads outside the chain launches),
    GCRL_SLAB_MEET (the slab's row groups exchange through a counter meeting): one child per switch runs its two SAC cases."""
    cases = [c for c in TABLE if c.proc == (switch,)]
    assert len(cases) == 2
    env = dict(os.environ)
    for k in gc.PROCESS_SWITCHES + gc.CREATION_SWITCHES:
        env.pop(k, None)
    env[switch] = "1"
    # this process waits in subprocess.run and launches nothing meanwhile, but its handles hold the per-device presence lock
    # (csrc/abi_misc.hip): the child would count the device as shared and run none of the forms these switches act on
    env["GCRL_NO_DEVICE_LOCK"] = "1"
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(_cus())] + [c.id for c in cases], capture_output=True, text=True, timeout=240,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    results = [json.loads(l[len("RESULT "):]) for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert [g["id"] for g in results] == [c.id for c in cases]
    for case, got in zip(cases, results):
        audit(case, got)
