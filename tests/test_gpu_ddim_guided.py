"""GPU (MI355X): guided DDIM with the built-in point objective as ONE library chain (cindm_ddpm1d_sample_ddim_guided), through the
public ``sample()`` / ``ddim_sample()``.

Expectations come from ``oracle/cindm_oracle.py::ddim_sample`` on the CPU at test time (pinned to the reference by
tests/golden/ddim_1d.npz: s10_guided_r2 and s10_guided_alpha_r1 restate at 0.0), with the same ``PointObjective`` differentiated by
autograd there and in closed form inside the update kernel here.  Tolerance: the project's chain tolerance (tests/test_gpu_parity.py,
TOL_CHAIN = 1e-4) on whole S = 10 chains and on teacher-forced segments of the S = 50 chain; the free-running S = 50 result is held
only to the 5e-2 of test_ddim_golden (the deterministic DDIM map amplifies a 1e-6 perturbation to 9e-4 at S = 50 with random-init
weights).

Objective coefficients (coef = 1 .. 2 on a state of order 1, targets inside [-1, 1]) were chosen by running the oracle cases on the
CPU first: every case has a gradient of the order of the state's own update (not identically zero -- asserted per case against the
unguided oracle chain or the objective's gradient at the result) and a final state that the clamp does not saturate everywhere
(asserted per case)."""
import pytest
import torch

import cindm_amd
import cindm_oracle as O
from cindm_amd import dist as cdist
from test_gpu_parity import TOL_CHAIN, build_unet, rel

pytestmark = pytest.mark.gpu

HZ = 24


def _say(name, v):
    print(f"[ddim-guided] {name}: {v:.3e}")
    return v


@pytest.fixture(scope="module")
def unet8(device):
    return build_unet(device)


def _diff(device, m, S, eta=0.0):
    return cindm_amd.GaussianDiffusion1D(m, image_size=HZ, conditioned_steps=0, timesteps=1000, sampling_timesteps=S,
                                         loss_type="l1", ddim_sampling_eta=eta).to(device)


def _tape(seed, shape, S, R, cond_shape=None):
    g = torch.Generator().manual_seed(seed)
    t = {"init": torch.randn(shape, generator=g), "step": torch.randn((S,) + tuple(shape), generator=g),
         "recur": torch.randn((S, R) + tuple(shape), generator=g)}
    if cond_shape is not None:
        t["cond"] = torch.randn((S,) + tuple(cond_shape), generator=g)
    return t


def _nt(t):
    return cindm_amd.NoiseTape(t["init"], t["step"], t["recur"], t.get("cond"))


def _not_degenerate(obj, ref):
    """The case exercises what it is meant to: the objective pulls on the result and the clamp leaves elements free."""
    x = ref.clone().requires_grad_()
    g = torch.autograd.grad(obj(x), x)[0]
    assert float(g.abs().max()) > 1e-3, "objective gradient vanishes on the oracle's result"
    assert float((ref.abs() < 1.0).float().mean()) > 0.25, "the clamp saturates (almost) every element"


class _NeverCalled(cindm_amd.PointObjective):
    def __call__(self, pos):
        raise AssertionError("the built-in route evaluated the objective in Python")


# name -> (S, eta, guidance, F, sample kwargs, objective kwargs, iso rows, inpaint rows)
CASES = {
    "r2": (10, 0.0, "standard-recurrence-2", 8, {}, dict(last_n_step=2, coef=2.0), 0, 0),
    "alpha_r1": (10, 0.3, "standard-alpha-recurrence-1", 8, {}, dict(last_n_step=3, coef=2.0, design_fn_mode="L2square"), 0, 0),
    "tc_l2_iso": (10, 0.0, "standard-recurrence-2", 8, {}, dict(last_n_step=2, coef=2.0, time_consistency_coef=0.5, design_fn_mode="L2"), 3, 0),
    "inpaint": (10, 0.5, "standard-recurrence-2", 8, {}, dict(last_n_step=2, coef=2.0), 0, 4),
    "nb4": (10, 0.0, "standard-recurrence-2", 16, dict(compose_n_bodies=4), dict(last_n_step=2, coef=1.0), 0, 0),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_chain_matches_oracle(device, unet8, name):
    """Item 1: tape-driven parity with the oracle, whole S = 10 chains, B = 2."""
    S, eta, guid, F, skw, okw, iso_rows, inp_rows = CASES[name]
    m, sd = unet8
    B, R = 2, int(guid.split("-")[-1])
    shape = (B, HZ, F)
    obj = _NeverCalled([0.25, -0.5], **okw)
    plain = cindm_amd.PointObjective([0.25, -0.5], **okw)
    g = torch.Generator().manual_seed(400 + len(name))
    iso = torch.randn((B, iso_rows, F), generator=g) * 0.3 if iso_rows else None
    cond = torch.rand((B, inp_rows, F), generator=g) * 2 - 1 if inp_rows else None
    tp = _tape(4100 + len(name), shape, S, R, None if cond is None else tuple(cond.shape))
    od = O.Diffusion1D(sd, image_size=HZ, conditioned_steps=0)
    kw = dict(n_composed=0, compose_mode="mean-inside", design_guidance=guid, **skw)
    ref = O.ddim_sample(od, shape, cond, tp, sampling_timesteps=S, eta=eta, design_fn=plain, initial_state_overwrite=iso, **kw)
    _not_degenerate(plain, ref)
    d = _diff(device, m, S, eta)
    dev = lambda t: None if t is None else t.to(device)
    out = d.ddim_sample(shape, dev(cond), design_fn=obj, initial_state_overwrite=dev(iso), noise=_nt(tp), **kw)
    assert tuple(out.shape) == shape
    assert _say(f"{name} vs oracle", rel(out, ref)) < TOL_CHAIN


def test_long_chain_teacher_forced(device, unet8):
    """Item 1, S = 50: the free-running result at test_ddim_golden's loose bound, parity on teacher-forced segments."""
    m, sd = unet8
    S, B, R, guid = 50, 2, 1, "standard-recurrence-1"
    shape = (B, HZ, 8)
    obj = cindm_amd.PointObjective([0.25, -0.5], 2, coef=2.0)
    tp = _tape(4200, shape, S, R)
    od = O.Diffusion1D(sd, image_size=HZ, conditioned_steps=0)
    kw = dict(n_composed=0, compose_mode="mean-inside", design_guidance=guid)
    states = {}
    ref = O.ddim_sample(od, shape, None, tp, sampling_timesteps=S, eta=0.0, design_fn=obj,
                        record=lambda i, img: states.__setitem__(i, img.clone()), **kw)
    _not_degenerate(obj, ref)
    d = _diff(device, m, S)
    out = d.sample(batch_size=B, design_fn=obj, noise=_nt(tp), **kw)
    assert _say("s50 free-running", rel(out, ref)) < 5e-2
    cks = [9, 19, 29, 39]
    for k, i in enumerate(cks):
        i_next = cks[k + 1] if k + 1 < len(cks) else S - 1
        seg = d.ddim_sample(shape, None, design_fn=obj, noise=_nt(tp), init_img=states[i].to(device),
                            step_range=(i + 1, i_next + 1), **kw)
        assert _say(f"s50 segment {i + 1}..{i_next}", rel(seg, states[i_next])) < TOL_CHAIN
    head = d.ddim_sample(shape, None, design_fn=obj, noise=_nt(tp), step_range=(0, 10), **kw)
    assert _say("s50 segment 0..9", rel(head, states[9])) < TOL_CHAIN


@pytest.mark.parametrize("guid,eta", [("standard-recurrence-2", 0.0), ("standard-alpha-recurrence-3", 0.4)])
def test_builtin_route_equals_generic_route(device, unet8, guid, eta):
    """Item 2: the closed-form gradient inside the captured step against autograd on the same callable between library calls."""
    m, _ = unet8
    S, B, R = 10, 3, int(guid.split("-")[-1])
    obj = cindm_amd.PointObjective([0.1, 0.2], 2, coef=2.0, time_consistency_coef=0.25)
    d = _diff(device, m, S, eta)
    tp = _tape(4300, (B, HZ, 8), S, R)
    kw = dict(batch_size=B, n_composed=0, compose_mode="mean-inside", design_guidance=guid)
    fast = d.sample(design_fn=obj, noise=_nt(tp), **kw)
    slow = d.sample(design_fn=lambda x: obj(x), noise=_nt(tp), **kw)
    assert _say(f"routes {guid}", rel(fast, slow)) < TOL_CHAIN


def test_bitwise_properties(device, unet8):
    """Item 3 (counter-based noise): graph == stream, batch split, seeds, the clamp of the last step, R = 1 and R = 3."""
    m, _ = unet8
    obj = cindm_amd.PointObjective([0.25, -0.5], 2, coef=2.0)
    d = _diff(device, m, 9, eta=1.0)              # (9 steps x 3 iterations: an odd iteration count, the result lands in the workspace buffer)
    for R in (1, 3):
        kw = dict(n_composed=0, compose_mode="mean-inside", design_fn=obj, design_guidance=f"standard-recurrence-{R}")
        a = d.sample(batch_size=64, seed=11, **kw)
        b = d.sample(batch_size=64, seed=11, use_graph=False, **kw)
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
        lo = d.sample(batch_size=32, seed=11, sample_offset=0, **kw)
        hi = d.sample(batch_size=32, seed=11, sample_offset=32, **kw)
        assert torch.equal(a, torch.cat([lo, hi]))
        assert torch.equal(a, d.sample(batch_size=64, seed=11, **kw))
        assert not torch.equal(a, d.sample(batch_size=64, seed=12, **kw))
        assert float(a.abs().max()) <= 1.0 + 1e-5            # the last DDIM step returns the clamped x_start
    d2 = _diff(device, m, 10, eta=1.0)            # an even count of steps and iterations
    kw = dict(n_composed=0, compose_mode="mean-inside", design_fn=obj, design_guidance="standard-alpha-recurrence-2")
    a = d2.sample(batch_size=8, seed=5, **kw)
    assert torch.equal(a, d2.sample(batch_size=8, seed=5, use_graph=False, **kw))
    assert torch.equal(a[4:], d2.sample(batch_size=4, seed=5, sample_offset=4, **kw))


def test_it_is_one_library_chain(device, unet8):
    """Item 4: the objective's Python side is never evaluated on the built-in route, and the chain answers for itself."""
    m, _ = unet8
    d = _diff(device, m, 10)
    obj = _NeverCalled([0.25, -0.5], 2, coef=2.0)
    out = d.sample(batch_size=4, n_composed=0, compose_mode="mean-inside", design_fn=obj,
                   design_guidance="standard-recurrence-2", seed=1)
    info = d.last_chain_info()
    assert tuple(out.shape) == (4, HZ, 8) and bool(torch.isfinite(out).all())
    assert info["chains_in_flight"] == 1 and not info["recovered"] and not info["exchange_free_up_front"]
    # one relaxation iteration = the U-Net's launches + one update launch, no counter launch: one launch more than the unguided DDIM
    # step, whose update runs inside the U-Net's last kernel and whose step state ping-pongs as well
    launches, fused = d.last_step_info()
    d.sample(batch_size=4, n_composed=0, seed=1)
    launches_unguided, fused_unguided = d.last_step_info()
    assert fused_unguided and not fused and launches == launches_unguided + 1, (launches, launches_unguided)
    with pytest.raises(AssertionError, match="in Python"):        # the generic routes do call it
        d.sample(batch_size=4, n_composed=0, compose_mode="mean-inside", design_fn=obj,
                 design_guidance="universal-forward-recurrence-2", seed=1)


def test_exchange_timeout_is_recovered_once(device):
    """Item 5: dbg = 39 stands in for a partner workgroup kept off the chip (test_gpu_ula.py's pattern): the chain is re-run once on the
    exchange-free kernels and equals what that selection computes by itself."""
    m, _ = build_unet(device)
    m.set_option("auto_range", 0)
    d = _diff(device, m, 6, eta=0.5)
    obj = cindm_amd.PointObjective([0.25, -0.5], 2, coef=2.0)
    run = lambda: d.sample(batch_size=6, n_composed=0, compose_mode="mean-inside", design_fn=obj,
                           design_guidance="standard-recurrence-2", seed=3)
    m.exchange_free(True)
    ref = run().clone()
    m.exchange_free(False)
    assert m.recovered == 0 and not d.last_chain_info()["recovered"]
    m.set_option("dbg", 39)
    try:
        got = run()
        info = d.last_chain_info()
    finally:
        m.set_option("dbg", 0)
    assert info["recovered"] and m.recovered == 1
    assert torch.equal(got, ref)


def test_sample_sharded_agrees_with_unsharded(device, unet8):
    """Item 6: dist.sample_sharded (a world of one) and the sample_offset form of a two-way split."""
    m, _ = unet8
    d = _diff(device, m, 8, eta=1.0)
    obj = _NeverCalled([0.25, -0.5], 2, coef=2.0)
    kw = dict(n_composed=0, compose_mode="mean-inside", design_fn=obj, design_guidance="standard-recurrence-2")
    whole = d.sample(batch_size=10, seed=21, **kw)
    assert torch.equal(cdist.sample_sharded(d, 10, seed=21, **kw), whole)
    parts = [d.sample(batch_size=hi - lo, seed=21, sample_offset=lo, **kw) for lo, hi in (cdist.shard_bounds(10, r, 2) for r in range(2))]
    assert torch.equal(torch.cat(parts), whole)
