"""GPU (MI355X): the waypoint objective (cindm_amd.WaypointObjective) inside the two captured guided chains
(cindm_ddpm1d_sample_guided / _sample_ddim_guided with descriptor modes 3 / 4 and cindm_ddpm1d_set_design_tables).

Expectations come from oracle/cindm_oracle.py on the CPU at test time, differentiating the SAME callable with autograd where the update
kernel evaluates the closed form from its two device tables.  Tolerances: tests/test_gpu_parity.py's TOL_STEP on single guided steps
and TOL_CHAIN on short whole chains.  The bitwise statements (table form == point form, broadcast == materialised, graph == stream,
shards == whole) hold by construction: the table branch has the point branch's expression order, and ``from_point`` forms the scale by
the one fp32 division the point branch does on the device.

Shapes: B = 2 / 3 (the design stride of per-design tables), L_tot = 56 (three windows, cs = 16) and 24, two and four bodies; every
table has zero and non-zero scales on every body and waypoints on row 0, on interior rows and on the last row.  Coefficients (scale
of order 1 .. 3 on a state of order 1 for the chains, 20 for single steps as test_gpu_parity's point cases) were chosen by running the
oracle cases on the CPU first: every chain case is guarded as test_gpu_ddim_guided._not_degenerate guards its own."""
import pytest
import torch

import cindm_amd
import cindm_oracle as O
from cindm_amd import _ffi
from cindm_amd import dist as cdist
from test_gpu_ddim_guided import _not_degenerate, _nt, _tape
from test_gpu_parity import TOL_CHAIN, TOL_STEP, build_unet, rel

pytestmark = pytest.mark.gpu

HZ = 24


def _say(name, v):
    print(f"[waypoint] {name}: {v:.3e}")
    return v


@pytest.fixture(scope="module")
def unet8(device):
    return build_unet(device)


@pytest.fixture(scope="module")
def diff8(device, unet8):
    return cindm_amd.GaussianDiffusion1D(unet8[0], image_size=HZ, conditioned_steps=0, timesteps=1000, sampling_timesteps=1000,
                                         loss_type="l1").to(device)


def _ddim(device, m, S, eta=0.0):
    return cindm_amd.GaussianDiffusion1D(m, image_size=HZ, conditioned_steps=0, timesteps=1000, sampling_timesteps=S,
                                         loss_type="l1", ddim_sampling_eta=eta).to(device)


def make_tables(seed, L, nb, B=None, per_target=False, per_weight=False):
    """(target, weight): waypoints on rows 0, 3, L // 3, L // 2 and L - 1 -- every body has entries that are zero and entries that
    are not on them, in another pattern per design -- and no waypoint anywhere else; targets inside [-0.6, 0.6]."""
    g = torch.Generator().manual_seed(seed)
    rows = [0, 3, L // 3, L // 2, L - 1]
    nd = B if B is not None else 1
    target = torch.rand((nd, L, nb, 2), generator=g) * 1.2 - 0.6
    weight = torch.zeros((nd, L, nb))
    for b in range(nd):
        for k, r in enumerate(rows):
            for j in range(nb):
                if (k + j + b) % 3 != 0:
                    weight[b, r, j] = 0.5 + float(torch.rand((), generator=g))
    for j in range(nb):
        on = weight[:, rows, j]
        assert bool((on == 0).any()) and bool((on > 0).any())
    assert nd == 1 or not torch.equal(target[0], target[1])
    return (target if per_target else target[0]).contiguous(), (weight if per_weight else weight[0]).contiguous()


def make_objective(seed, L, nb, B=None, per_target=False, per_weight=False, cls=cindm_amd.WaypointObjective, **kw):
    target, weight = make_tables(seed, L, nb, B, per_target, per_weight)
    return cls(target, weight, **kw)


class _NeverCalled(cindm_amd.WaypointObjective):
    def __call__(self, pos):
        raise AssertionError("the built-in route evaluated the objective in Python")


# ------------------------------------------------------------------ 1. one guided step against the oracle
# (guidance, mode, tc, target per design, weight per design, initial_state_overwrite): every value of every factor, each pair of
# guidance x mode, and both mixed per-design forms (the two flag bits of the kernel's mode word apart)
STEP_CASES = [("standard", "L2", 0.0, False, False, False), ("standard", "L2square", 0.5, True, True, True),
              ("standard-alpha", "L2", 0.5, True, False, False), ("standard-alpha", "L2square", 0.0, False, False, True),
              ("standard-recurrence-2", "L2", 0.5, False, False, True), ("standard-recurrence-2", "L2square", 0.0, False, True, False),
              ("standard-alpha-recurrence-3", "L2", 0.0, True, True, True), ("standard-alpha-recurrence-3", "L2square", 0.5, False, False, False)]


@pytest.mark.parametrize("guid,mode,tc,ptarget,pweight,use_iso", STEP_CASES)
def test_step_vs_oracle(device, unet8, diff8, guid, mode, tc, ptarget, pweight, use_iso):
    """One guided reverse step (3 windows, mean-inside, L_tot = 56) at t = 600, 30, 0; the overwrite covers rows 0 .. 3, which carry
    waypoints (rows 0 and 3)."""
    _, sd = unet8
    B, L, F = 2, 56, 8
    od = O.Diffusion1D(sd, image_size=HZ, conditioned_steps=0)
    obj = make_objective(11, L, 2, B, ptarget, pweight, cls=_NeverCalled, coef=20.0, time_consistency_coef=tc, design_fn_mode=mode)
    plain = make_objective(11, L, 2, B, ptarget, pweight, coef=20.0, time_consistency_coef=tc, design_fn_mode=mode)
    R = int(guid.split("-")[-1]) if "recurrence" in guid else 0
    g = torch.Generator().manual_seed(21)
    kw = dict(compose_mode="mean-inside", n_composed=2, compose_start_step=16, single_model_step=HZ, compose_n_bodies=2)
    desc = diff8._desc_for((B, L, F), "mean-inside", 2, 16, HZ, 2)
    for t in (600, 30, 0):
        x = torch.randn((B, L, F), generator=g) * 0.7
        nz = torch.randn((B, L, F), generator=g)
        rn = torch.randn((max(R, 1), B, L, F), generator=g)
        iso = torch.randn((B, 4, F), generator=g) * 0.3 if use_iso else None
        ref, _ = O.p_sample_compose_inside(od, x.clone(), None, t, nz, design_fn=plain, design_guidance=guid, recur_noise=rn,
                                           initial_state_overwrite=iso, **kw)
        if R == 0 and t == 600:           # the gradient moves the step by far more than the tolerance
            unguided, _ = O.p_sample_compose_inside(od, x.clone(), None, t, nz, design_guidance=guid, initial_state_overwrite=iso, **kw)
            assert rel(unguided, ref) > 100 * TOL_STEP
        step = torch.zeros((1000, B, L, F)); step[t] = nz
        rec = torch.zeros((1000, max(R, 1), B, L, F)); rec[t] = rn
        tape = cindm_amd.NoiseTape(None, step, rec).to(device)
        out = diff8._run_guided_loop(x.clone().to(device), None, desc, obj.descriptor(guid), t, t, noise=tape, seed=0, sample_offset=0,
                                     inpaint_cond=None, initial_state_overwrite=None if iso is None else iso.to(device), tables=obj)
        assert _say(f"step {guid} {mode} t={t}", rel(out, ref)) < TOL_STEP, (guid, t)


# ------------------------------------------------------------------ 2. short whole chains against the oracle
def test_ddpm_chain_vs_oracle(device, unet8, diff8):
    """t = 999 .. 985, B = 3, one composed window more (L_tot = 40, cs = 16), per-design tables."""
    _, sd = unet8
    B, L = 3, 40
    kwo = dict(coef=2.0, time_consistency_coef=0.25)
    obj = make_objective(31, L, 2, B, True, True, cls=_NeverCalled, **kwo)
    plain = make_objective(31, L, 2, B, True, True, **kwo)
    tape = O.NoiseTape.make(92, (B, L, 8), 1000, recur=2)
    od = O.Diffusion1D(sd, image_size=HZ, conditioned_steps=0)
    kw = dict(n_composed=1, compose_start_step=16, compose_mode="mean-inside", design_guidance="standard-recurrence-2", t_stop=985)
    ref = O.sample(od, B, tape, design_fn=plain, **kw)
    _not_degenerate(plain, ref)
    out = diff8.sample(batch_size=B, design_fn=obj, noise=cindm_amd.NoiseTape(tape.init, tape.step, tape.recur), **kw)
    assert tuple(out.shape) == (B, L, 8)
    assert _say("ddpm chain vs oracle", rel(out, ref)) < TOL_CHAIN


# name -> (eta, guidance, n_bodies, mode, tc, per-design, iso rows, inpaint rows)
DDIM_CASES = {
    "nb2": (0.0, "standard-recurrence-2", 2, "L2", 0.5, True, 3, 0),
    "nb2_sq_alpha": (0.3, "standard-alpha-recurrence-1", 2, "L2square", 0.0, False, 0, 0),
    "nb2_inpaint": (0.5, "standard-recurrence-2", 2, "L2", 0.0, True, 0, 4),
    "nb4": (0.0, "standard-recurrence-2", 4, "L2", 0.0, True, 0, 0),
}


def ddim_case(name):
    """(objective kwargs, table arguments, oracle / sample kwargs, tape, cond, iso) of a DDIM chain case: S = 10, B = 2, L_tot = 24."""
    eta, guid, nb, mode, tc, per, iso_rows, inp_rows = DDIM_CASES[name]
    S, B, R, F = 10, 2, int(guid.split("-")[-1]), 4 * nb
    shape = (B, HZ, F)
    g = torch.Generator().manual_seed(500 + len(name))
    iso = torch.randn((B, iso_rows, F), generator=g) * 0.3 if iso_rows else None
    cond = torch.rand((B, inp_rows, F), generator=g) * 2 - 1 if inp_rows else None
    tp = _tape(5100 + len(name), shape, S, R, None if cond is None else tuple(cond.shape))
    okw = dict(coef=1.0 if nb == 4 else 2.0, time_consistency_coef=tc, design_fn_mode=mode)
    kw = dict(n_composed=0, compose_mode="mean-inside", design_guidance=guid, **({"compose_n_bodies": 4} if nb == 4 else {}))
    return S, eta, shape, okw, (41 + nb, HZ, nb, B, per, per), kw, tp, cond, iso


@pytest.mark.parametrize("name", sorted(DDIM_CASES))
def test_ddim_chain_vs_oracle(device, unet8, name):
    S, eta, shape, okw, targs, kw, tp, cond, iso = ddim_case(name)
    m, sd = unet8
    obj, plain = make_objective(*targs, cls=_NeverCalled, **okw), make_objective(*targs, **okw)
    od = O.Diffusion1D(sd, image_size=HZ, conditioned_steps=0)
    ref = O.ddim_sample(od, shape, cond, tp, sampling_timesteps=S, eta=eta, design_fn=plain, initial_state_overwrite=iso, **kw)
    _not_degenerate(plain, ref)
    d = _ddim(device, m, S, eta)
    dev = lambda t: None if t is None else t.to(device)
    out = d.ddim_sample(shape, dev(cond), design_fn=obj, initial_state_overwrite=dev(iso), noise=_nt(tp), **kw)
    assert tuple(out.shape) == shape
    assert _say(f"ddim {name} vs oracle", rel(out, ref)) < TOL_CHAIN


# ------------------------------------------------------------------ 3. table form == point form, bit for bit
@pytest.mark.parametrize("mode", ["L2", "L2square"])
def test_table_form_equals_point_form(device, unet8, diff8, mode):
    m, _ = unet8
    okw = dict(coef=1.0, time_consistency_coef=0.5, design_fn_mode=mode)          # (1 / 3: the scale is not exact in fp32)
    point = cindm_amd.PointObjective([0.25, -0.5], 3, **okw)
    tape = O.NoiseTape.make(93, (3, 40, 8), 1000, recur=2)
    kw = dict(batch_size=3, n_composed=1, compose_start_step=16, compose_mode="mean-inside", design_guidance="standard-recurrence-2",
              noise=cindm_amd.NoiseTape(tape.init, tape.step, tape.recur), t_stop=990)
    a = diff8.sample(design_fn=point, **kw)
    b = diff8.sample(design_fn=cindm_amd.WaypointObjective.from_point([0.25, -0.5], 3, 40, 2, **okw), **kw)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    okw["coef"] = 2.0
    point = cindm_amd.PointObjective([0.25, -0.5], 3, **okw)
    d = _ddim(device, m, 10, eta=0.5)
    tp = _tape(5300, (2, HZ, 8), 10, 2)
    kw = dict(batch_size=2, n_composed=0, compose_mode="mean-inside", design_guidance="standard-alpha-recurrence-2")
    a = d.sample(design_fn=point, noise=_nt(tp), **kw)
    b = d.sample(design_fn=cindm_amd.WaypointObjective.from_point([0.25, -0.5], 3, HZ, 2, **okw), noise=_nt(tp), **kw)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    assert not torch.equal(a, d.sample(design_fn=cindm_amd.WaypointObjective.from_point([0.25, -0.4], 3, HZ, 2, **okw), noise=_nt(tp), **kw))


# ------------------------------------------------------------------ 4. broadcast == materialised
def test_broadcast_equals_materialised(device, unet8):
    m, _ = unet8
    B = 3
    d = _ddim(device, m, 10, eta=0.5)
    target, weight = make_tables(61, HZ, 2)
    kwo = dict(coef=2.0, time_consistency_coef=0.25)
    kw = dict(batch_size=B, n_composed=0, compose_mode="mean-inside", design_guidance="standard-recurrence-2", seed=17)
    shared = d.sample(design_fn=cindm_amd.WaypointObjective(target, weight, **kwo), **kw)
    for tt, ww in ((target.expand(B, -1, -1, -1), weight.expand(B, -1, -1)), (target.expand(B, -1, -1, -1), weight),
                   (target, weight.expand(B, -1, -1))):
        assert torch.equal(d.sample(design_fn=cindm_amd.WaypointObjective(tt.contiguous(), ww.contiguous(), **kwo), **kw), shared)


# ------------------------------------------------------------------ 5. routes
@pytest.mark.parametrize("guid,eta", [("standard-recurrence-2", 0.0), ("standard-alpha-recurrence-3", 0.4)])
def test_builtin_route_equals_generic_route(device, unet8, diff8, guid, eta):
    m, _ = unet8
    B, R = 3, int(guid.split("-")[-1])
    obj = make_objective(71, HZ, 2, B, True, True, coef=2.0, time_consistency_coef=0.25)
    d = _ddim(device, m, 10, eta)
    tp = _tape(5400, (B, HZ, 8), 10, R)
    kw = dict(batch_size=B, n_composed=0, compose_mode="mean-inside", design_guidance=guid)
    fast = d.sample(design_fn=obj, noise=_nt(tp), **kw)
    slow = d.sample(design_fn=lambda x: obj(x), noise=_nt(tp), **kw)
    assert bool(torch.isfinite(slow).all())
    assert _say(f"routes ddim {guid}", rel(fast, slow)) < TOL_CHAIN
    # DDPM, t = 999 .. 992, without "-alpha": there eta_t = beta_t / sqrt(abar_{t-1}) is ~2e4 on the cosine schedule and the unclamped
    # DDPM state overflows on BOTH routes within these steps (the time-consistency term is linear in the state); the DDIM chain above
    # rebuilds its state from the clamped x_start every step and carries the alpha case
    guid = guid.replace("-alpha", "")
    obj40 = make_objective(72, 40, 2, B, True, True, coef=2.0, time_consistency_coef=0.25)
    tape = O.NoiseTape.make(94, (B, 40, 8), 1000, recur=R)
    kw = dict(batch_size=B, n_composed=1, compose_start_step=16, compose_mode="mean-inside", design_guidance=guid,
              noise=cindm_amd.NoiseTape(tape.init, tape.step, tape.recur), t_stop=992)
    fast = diff8.sample(design_fn=obj40, **kw)
    slow = diff8.sample(design_fn=lambda x: obj40(x), **kw)
    assert bool(torch.isfinite(slow).all())
    assert _say(f"routes ddpm {guid}", rel(fast, slow)) < TOL_CHAIN


def test_library_chain_properties(device, unet8, diff8):
    """The objective's Python side is never evaluated; graph == stream; two half-batches with shard + sample_offset == the whole batch
    (counter-based draws), through sample_sharded's own path as well."""
    m, _ = unet8
    B = 4
    d = _ddim(device, m, 9, eta=1.0)            # (9 steps x 3 iterations: odd, the result lands in the workspace buffer)
    obj = make_objective(81, HZ, 2, B, True, True, cls=_NeverCalled, coef=2.0)
    kw = dict(n_composed=0, compose_mode="mean-inside", design_guidance="standard-recurrence-3")
    whole = d.sample(batch_size=B, design_fn=obj, seed=11, **kw)
    assert bool(torch.isfinite(whole).all())
    assert torch.equal(whole, d.sample(batch_size=B, design_fn=obj, seed=11, use_graph=False, **kw))
    parts = [d.sample(batch_size=hi - lo, design_fn=obj.shard(lo, hi), seed=11, sample_offset=lo, **kw) for lo, hi in ((0, 2), (2, 4))]
    assert torch.equal(torch.cat(parts), whole)
    assert not torch.equal(parts[0], parts[1])
    assert torch.equal(cdist.sample_sharded(d, B, seed=11, design_fn=obj, **kw), whole)
    with pytest.raises(AssertionError, match="in Python"):        # the generic routes do call it
        d.sample(batch_size=B, design_fn=obj, seed=11, n_composed=0, compose_mode="mean-inside",
                 design_guidance="universal-forward-recurrence-2")
    obj40 = make_objective(82, 40, 2, B, True, True, cls=_NeverCalled, coef=0.2, design_fn_mode="L2square")
    kw = dict(n_composed=1, compose_start_step=16, compose_mode="mean-inside", design_guidance="standard", t_stop=992)
    whole = diff8.sample(batch_size=B, design_fn=obj40, seed=12, **kw)
    assert bool(torch.isfinite(whole).all())
    assert torch.equal(whole, diff8.sample(batch_size=B, design_fn=obj40, seed=12, use_graph=False, **kw))
    parts = [diff8.sample(batch_size=2, design_fn=obj40.shard(lo, lo + 2), seed=12, sample_offset=lo, **kw) for lo in (0, 2)]
    assert torch.equal(torch.cat(parts), whole)


# ------------------------------------------------------------------ 6. graph reuse
def test_graph_follows_the_tables(device, unet8):
    """A and B are alive together on one handle, so their device tables have other addresses: the table addresses are part of the
    graph key, B captures its own step, and the same A afterwards gives A's designs again."""
    m, _ = unet8
    d = _ddim(device, m, 6, eta=0.5)
    kw = dict(batch_size=2, n_composed=0, compose_mode="mean-inside", design_guidance="standard-recurrence-2", seed=5)
    A, B_ = (make_objective(seed, HZ, 2, 2, True, True, coef=2.0) for seed in (91, 92))
    a1 = d.sample(design_fn=A, **kw).clone()
    b = d.sample(design_fn=B_, **kw).clone()
    a2 = d.sample(design_fn=A, **kw)
    (ta, sa), (tb, sb) = A.tables(device), B_.tables(device)
    assert ta.data_ptr() != tb.data_ptr() and sa.data_ptr() != sb.data_ptr()
    assert torch.equal(a1, a2) and not torch.equal(a1, b)
    # B's designs are those of a handle that has never seen A
    assert torch.equal(b, _ddim(device, m, 6, eta=0.5).sample(design_fn=make_objective(92, HZ, 2, 2, True, True, coef=2.0), **kw))


# ------------------------------------------------------------------ 7. recorder
def test_recorder_on_the_table_route(device, unet8, diff8):
    m, _ = unet8
    d = _ddim(device, m, 10, eta=0.5)
    obj = make_objective(95, HZ, 2, 2, True, True, cls=_NeverCalled, coef=2.0)
    kw = dict(batch_size=2, n_composed=0, compose_mode="mean-inside", design_fn=obj, design_guidance="standard-recurrence-2", seed=7)
    out, rec = d.sample(return_trajectory_every=3, trajectory=("x", "x0"), **kw)
    assert rec.step == [3, 6, 9, 10] and tuple(rec.x.shape) == (4, 2, HZ, 8) == tuple(rec.x0.shape)
    assert torch.equal(rec.x[-1], out) and torch.equal(out, d.sample(**kw))
    obj40 = make_objective(96, 40, 2, 2, True, True, cls=_NeverCalled, coef=2.0)
    kw = dict(batch_size=2, n_composed=1, compose_start_step=16, compose_mode="mean-inside", design_fn=obj40,
              design_guidance="standard-recurrence-2", seed=7, t_stop=993)
    out, rec = diff8.sample(return_trajectory_every=3, trajectory=("x", "x0"), **kw)
    assert rec.t == [997, 994, 993] and torch.equal(rec.x[-1], out) and torch.equal(out, diff8.sample(**kw))


# ------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_handle_usable(device, unet8, diff8):
    B, L = 2, 40
    obj = make_objective(97, L, 2, B, True, True, coef=2.0)
    point = cindm_amd.PointObjective([0.25, -0.5], 2, coef=2.0)
    guid = "standard-recurrence-2"
    desc = diff8._desc_for((B, L, 8), "mean-inside", 1, 16, HZ, 2)
    x0 = torch.randn((B, L, 8), generator=torch.Generator().manual_seed(1)).to(device)
    run = lambda dz, tables: diff8._run_guided_loop(x0.clone(), None, desc, dz, 999, 998, noise=None, seed=3, sample_offset=0,
                                                    inpaint_cond=None, initial_state_overwrite=None, tables=tables)
    good = run(obj.descriptor(guid), obj)
    with pytest.raises(cindm_amd.CindmError, match="arm them with cindm_ddpm1d_set_design_tables"):
        run(obj.descriptor(guid), None)                                  # mode 3, nothing armed
    assert torch.equal(run(obj.descriptor(guid), obj), good)
    with pytest.raises(cindm_amd.CindmError, match="the descriptor's mode is 1 / 2"):
        run(point.descriptor(guid), obj)                                 # armed tables, point descriptor
    assert torch.equal(run(obj.descriptor(guid), obj), good)
    wrong = make_objective(97, L + 16, 2, B, True, True, coef=2.0)
    with pytest.raises(cindm_amd.CindmError, match="56 rows, the state has 40"):
        run(wrong.descriptor(guid), wrong)                               # the library's own check
    with pytest.raises(cindm_amd.CindmError, match="batch of 3"):
        run(obj.descriptor(guid), make_objective(97, L, 2, 3, True, True, coef=2.0))
    kw = dict(batch_size=B, n_composed=1, compose_start_step=16, compose_mode="mean-inside", design_guidance=guid, seed=3, t_stop=998)
    for bad in (wrong, make_objective(97, L, 4, B, True, True), make_objective(97, L, 2, 3, True, True)):
        with pytest.raises(ValueError, match="WaypointObjective"):       # the public route refuses before any device work
            diff8.sample(design_fn=bad, **kw)
    # armed tables on a chain that is not guided: refused, consumed, and the next unguided chain runs
    obj.arm(diff8._handle(), B, device)
    with pytest.raises(cindm_amd.CindmError, match="only the guided chains"):
        diff8.sample(batch_size=B, n_composed=0, seed=3, t_stop=998)
    assert bool(torch.isfinite(diff8.sample(batch_size=B, n_composed=0, seed=3, t_stop=998)).all())
    h = diff8._handle()
    t, s = obj.tables(device)
    assert _ffi.lib().cindm_ddpm1d_set_design_tables(h, _ffi.ptr(t), 1, None, 1, L, 2, B) != 0      # one table without the other
    _ffi.check(_ffi.lib().cindm_ddpm1d_set_design_tables(h, _ffi.ptr(t), 1, _ffi.ptr(s), 1, L, 2, B))
    _ffi.check(_ffi.lib().cindm_ddpm1d_set_design_tables(h, None, 0, None, 0, 0, 0, 0))              # disarm
    assert bool(torch.isfinite(diff8.sample(batch_size=B, n_composed=0, seed=3, t_stop=998)).all())
    assert torch.equal(run(obj.descriptor(guid), obj), good)
    assert bool(torch.isfinite(diff8.sample(design_fn=obj, **kw)).all())


def test_2d_entries_refuse_armed_tables(device):
    """The four 2-D chain entries take armed waypoint tables like everything else that is armed, and refuse them: the call fails with
    the tables' message, and the same call passes afterwards -- the refused call consumed the tables."""
    from test_gpu_multistep import CH, HW, _diff2, _force_objective          # (that module imports this one)
    from test_gpu_parity_2d import build_unet2d
    unet2d = build_unet2d(device)
    force = cindm_amd.ForceUnet(dim=64, dim_mults=(1, 2, 4, 8), channels=4)
    force.load_state_dict(O.synth_state_dict_2d(O.force_unet_param_shapes(), 7), strict=True)
    force = force.to(device)
    shape = (1, 2, CH, HW, HW)
    fn = _force_objective(force, 1, 2)
    target, scale = torch.zeros((2, 4, 2, 2), device=device), torch.ones((2, 4, 2), device=device)      # batch 2, 4 rows, 2 bodies

    def armed_refusal(d, run):
        _ffi.check(_ffi.lib().cindm_ddpm1d_set_design_tables(d._handle(), _ffi.ptr(target), 1, _ffi.ptr(scale), 1, 4, 2, 2))
        with pytest.raises(cindm_amd.CindmError, match="design tables: only the guided chains"):
            run()
        assert bool(torch.isfinite(run()).all())

    d = _diff2(device, unet2d, 1000)
    armed_refusal(d, lambda: d.p_sample_loop(shape, seed=1, t_stop=998))                                  # cindm_ddpm2d_sample
    armed_refusal(d, lambda: d.p_sample_loop(shape, fn, "standard-alpha", seed=1, t_stop=998))            # _sample_force
    d2 = _diff2(device, unet2d, 2)
    armed_refusal(d2, lambda: d2.ddim_sample(shape, seed=1))                                              # _sample_ddim
    armed_refusal(d2, lambda: d2.ddim_sample(shape, fn, "standard-alpha", seed=1))                        # _sample_ddim_force
