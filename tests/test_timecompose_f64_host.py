"""CPU: the float64 statements of one step of the parallel time composition and of one Langevin update in oracle/f64_reference.py
(``timecompose_step_f64``, ``ula_update_f64``) are proven before they judge a kernel.

Over the whole grid of tests/timecompose_cases.py -- the one tests/test_gpu_timecompose_f64.py runs the library on -- the fp32 oracle's
own loop (``test_time_compose_host.restated_loop``; ``test_ula_host.restated_step_ula`` for the Langevin update) lies within
(n_e + 4) * 2^-24 * A_e of the statement on every element of every step, the statement evaluated on the oracle's OWN U-Net outputs (a
recorder around ``Diffusion1D.model`` / ``model_unconditioned``).  The restated loop is pinned to the reference project by
tests/golden/time_compose_parallel.npz and, for pred_x0 / pred_v with the clamp on, by tests/golden/time_compose_objectives.npz
(tests/manual/make_golden_time_compose.py), where at least 0.5 % of x_start lies on the clamp at every step that uses pred_noise.

Each mutation of the statement leaves the bound by FLOOR = 100 x at least on the steps listed for it (the smallest multiple each
reaches is in MUTATION_FACTORS).  The time composition's: pred_noise of the unclamped x_start (the defect the grid was written
for), the hand-over from a state one step older, to segment k, of the first Lc rows, the neighbouring segment's draw, san and c swapped,
the last pair not returning x_start, and for ``multibody`` the pair index, the slot and uncond_coef 1.0.  The Langevin update's: the sign
of the score, ss and std swapped, the draw of iteration l + 1, the unscaled score above t = 400 and the scaled one at or below it.

The Langevin tables: ``schedule.ula_schedule``'s fp32 entries are the float64 formulas' values rounded once, and those are the
correctly rounded values of the exact expressions (50-digit decimal arithmetic) for every timestep of linear_beta_schedule(1000).

``seg_magic``: (row * ceil(2^32 / B)) >> 32 == row // B on both sides of every multiple of B, for every B the entry admits.

The hand-over reaches a step through the rows the U-Net sees and through nothing else, so its mutations are made on those rows: the
statement is evaluated on the oracle's U-Net outputs of the mutated rows, and the recorder asserts that the un-mutated rows are the
ones the oracle's U-Net saw, bit for bit.

Largest ratio of the un-mutated statements: 0.3316 over the 66 chains of the time-composition grid (pred_x0, clamp on, eta 0.5, K = 3,
B = 5; the 8-step diffusion of SMALL_T = 8 stays at 0.2735), 0.2307 over the Langevin cases (two iterations at t = 400)."""
import decimal
import os

import numpy as np
import pytest
import torch

import cindm_oracle as O
import f64_reference as R
import timecompose_cases as T
from cindm_amd.schedule import ddim_schedule, ula_schedule
from step1d_cases import frozen_state_dict
from test_time_compose_host import restated_loop
from test_ula_host import linear_beta_schedule, restated_step_ula, scalar_for_gradient

FLOOR = 100.0
_TAB, _SD, _GOT = {}, {}, {}


def tab(case):
    key = (case.T, case.objective)
    if key not in _TAB:
        _TAB[key] = O.make_schedule("cosine", case.T, case.objective)
    return _TAB[key]


def _sd(hz, F, frozen=False):
    if (hz, F, frozen) not in _SD:
        sd = O.synth_state_dict(O.unet1d_param_shapes(hz, F, attention=True), seed=1 if F == 4 else 0)
        _SD[(hz, F, frozen)] = frozen_state_dict(sd) if frozen else sd
    return _SD[(hz, F, frozen)]


def ddim_rows(case):
    """fp32 [S, 3] (sqrt(alpha_next), c, sigma), as the library's chain is handed them."""
    import types
    shim = types.SimpleNamespace(num_timesteps=case.T, sampling_timesteps=case.S, ddim_sampling_eta=case.eta,
                                 alphas_cumprod=tab(case)["alphas_cumprod"])
    return ddim_schedule(shim)[1]


def _recorded(od):
    """Record every U-Net call of an oracle diffusion: -> (pair outputs, single-body outputs), lists in call order."""
    pair, single = [], []
    sd, su = od.sd, od.sd_uncond
    od.seen_in = []

    def model(x, t):
        od.seen_in.append(x.clone())
        pair.append(O.unet1d_forward(sd, x, t))
        return pair[-1]

    def model_unconditioned(x, t):
        single.append(O.unet1d_forward(su, x, t))
        return single[-1]
    od.model, od.model_unconditioned = model, model_unconditioned
    return pair, single


def oracle(case):
    """(states [S, K, B, R, F], x_starts [S, ...], [(E, U)] per step) of the fp32 oracle's loop on a case."""
    if case.index in _GOT:
        return _GOT[case.index]
    d = T.inputs(case)
    od = O.Diffusion1D(_sd(case.hz, 8), image_size=case.R, conditioned_steps=case.Lc, objective=case.objective, timesteps=case.T,
                       sd_uncond=_sd(case.hz, 4) if case.multibody else None)
    pair, single = _recorded(od)
    x0s = []
    states = restated_loop(od, d["cond"], d["init"], d["step"], case.S, case.eta, clip=case.clip, x_starts=x0s)
    assert len(pair) == case.S and len(single) == (4 * case.S if case.multibody else 0)
    for i in range(case.S):                   # the oracle's U-Net saw exactly the rows the statement is evaluated on
        assert torch.equal(od.seen_in[i], T.unet_rows(case, d, states, i)[0]), (case.name, i)
    outs = [T.shape_outputs(case, pair[i], torch.stack(single[4 * i:4 * i + 4]) if case.multibody else None) for i in range(case.S)]
    _GOT[case.index] = (states, torch.stack(x0s), outs)
    return _GOT[case.index]


def step_ratio(case, i, mut=None):
    """(ratio of the state, ratio of x_start, the statement) of step i."""
    states, x0s, outs = oracle(case)
    E, U = outs[i]
    if mut and any(m.startswith("handover") for m in mut):          # the hand-over reaches a step through the U-Net's rows alone
        pair_in, single_in = T.unet_rows(case, T.inputs(case), states, i, mut)
        tt = lambda rows: torch.full((rows.shape[0],), case.times()[i][0], dtype=torch.long)
        assert not case.multibody
        E, U = T.shape_outputs(case, O.unet1d_forward(_sd(case.hz, 8), pair_in, tt(pair_in)), None)
    st = T.statement(case, T.inputs(case), states, i, E, U, tab(case), ddim_rows(case)[i], mut=mut)
    return T.ratio(states[i], st["state"])[0], T.ratio(x0s[i], st["x_start"])[0], st


# ------------------------------------------------------------------ the grid, the fp32 oracle
@pytest.mark.parametrize("kind,objective", T.GROUPS, ids=[f"{k}-{o}" for k, o in T.GROUPS])
def test_oracle_within_bound(kind, objective):
    cases = [c for c in T.CASES if (c.kind, c.objective) == (kind, objective)]
    assert cases
    for c in cases:
        d, (states, _, outs) = T.inputs(c), oracle(c)
        worst, shares = 0.0, []
        for i in range(c.S):
            # the U-Net saw exactly the rows the statement assumes: the hand-over from the state before the step
            rs, r0, st = step_ratio(c, i)
            worst = max(worst, rs, r0)
            shares.append(T.clamp_share(st))
            assert rs <= 1.0 and r0 <= 1.0, (c.name, i, rs, r0)
        print(f"{c.name}: largest err/bound {worst:.4f}, clamp share {min(shares):.3f} .. {max(shares):.3f}")
        assert float(states[:-1].abs().max()) > 1.0


def test_grid_covers_the_axes():
    C = T.CASES
    grid = [c for c in C if c.kind == "grid"]
    assert {(c.objective, c.clip, c.eta, (c.K, c.B)) for c in grid} == {(o, cl, e, kb) for o in T.OBJECTIVES for cl in (True, False)
                                                                        for e in (0.0, 0.5) for kb in T.KB}
    threads = {(c.K, c.B): c.K * c.B * c.R * c.F // 4 for c in grid}
    assert threads[(3, 5)] == 600 and threads[(2, 16)] % 256 == 0 and threads[(4, 7)] % 256 != 0 and threads[(2, 1)] < 256
    assert {(c.objective, c.eta) for c in C if c.kind == "whole"} == {(o, e) for o in T.OBJECTIVES for e in (0.0, 0.5)}
    assert all(c.R == c.Lc for c in C if c.kind == "whole")
    assert {(c.objective, c.clip) for c in C if c.multibody} == {(o, cl) for o in T.OBJECTIVES for cl in (True, False)}
    small = [c for c in C if c.kind == "small"]
    assert {(c.objective, c.eta) for c in small} == {(o, e) for o in T.OBJECTIVES for e in (0.0, 0.5)}
    assert small[0].times()[-2:] == [(1, 0), (0, -1)] and len(small[0].times()) == T.SMALL_T
    assert grid[0].times()[0] == (999, 899) and grid[0].times()[-1] == (99, -1)


def test_clamp_bites_where_the_defect_lives():
    """pred_x0 / pred_v with the clamp on: part of x_start sits on the clamp at the steps that use pred_noise, so the re-derived noise
    differs from the unclamped one there."""
    for obj in ("pred_x0", "pred_v"):
        c = T.BY_NAME[f"grid-K3B5-{obj}-clip1-eta0.0"]
        shares = [T.clamp_share(step_ratio(c, i)[2]) for i in range(c.S - 1)]
        print(obj, [round(s, 4) for s in shares])
        assert max(shares) >= 0.005, (obj, shares)


# ------------------------------------------------------------------ the bound means something
def _steps(name, steps):
    return [(T.BY_NAME[name], i) for i in steps]


def _clamped_steps(name):
    """The steps of a case that use pred_noise and have x_start on the clamp."""
    c = T.BY_NAME[name]
    return [(c, i) for i in range(c.S - 1) if T.clamp_share(step_ratio(c, i)[2]) > 0]


MUTATIONS = {
    # (not the pair at t = 999: c there is 0.03 and the difference reaches 40 x only, as in the unguided DDIM chain)
    "eps_unclamped": lambda: _clamped_steps("grid-K3B5-pred_x0-clip1-eta0.0")[1:] + _clamped_steps("grid-K4B7-pred_v-clip1-eta0.5")[1:],
    "handover_older": lambda: _steps("grid-K3B5-pred_noise-clip1-eta0.5", (1, 5, 9)) + _steps("whole-K4B5-pred_x0-clip1-eta0.0", (2,)),
    "handover_same": lambda: _steps("grid-K3B5-pred_noise-clip1-eta0.5", (0, 5, 9)) + _steps("grid-K4B7-pred_v-clip0-eta0.0", (3,)),
    "handover_first": lambda: _steps("grid-K3B5-pred_noise-clip1-eta0.5", (0, 5, 9)) + _steps("grid-K2B16-pred_x0-clip0-eta0.0", (3,)),
    "noise_neighbour": lambda: _steps("grid-K3B5-pred_noise-clip1-eta0.5", (0, 5, 8)) + _steps("small-K3B5-pred_v-clip1-eta0.5", (6,)),
    "san_c_swap": lambda: _steps("grid-K3B5-pred_noise-clip1-eta0.0", (0, 5, 8)) + _steps("grid-K2B1-pred_v-clip0-eta0.5", (4,)),
    "last_not_x0": lambda: _steps("grid-K3B5-pred_noise-clip1-eta0.0", (9,)) + _steps("small-K3B5-pred_x0-clip1-eta0.5", (7,))
    + _steps("multibody-K2B3-pred_noise-clip1-eta0.5", (9,)),
    "pair_index": lambda: _steps("multibody-K2B3-pred_noise-clip1-eta0.5", (0, 5, 9)) + _steps("multibody-K2B3-pred_v-clip0-eta0.5", (4,)),
    "slot": lambda: _steps("multibody-K2B3-pred_noise-clip1-eta0.5", (0, 5, 9)) + _steps("multibody-K2B3-pred_x0-clip1-eta0.5", (4,)),
    "coef_1": lambda: _steps("multibody-K2B3-pred_noise-clip1-eta0.5", (0, 5, 9)) + _steps("multibody-K2B3-pred_v-clip1-eta0.5", (4,)),
}
# which elements a mutation touches: every segment but the first for the hand-over, every one but the last for the neighbour's draw
_TOUCHED = {"handover_older": slice(1, None), "handover_same": slice(1, None), "handover_first": slice(1, None), "noise_neighbour": slice(0, -1)}


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_mutation_leaves_the_bound(mut):
    cases = MUTATIONS[mut]()
    assert cases
    worst = float("inf")
    for c, i in cases:
        states, _, _ = oracle(c)
        good = step_ratio(c, i)[0]
        st = step_ratio(c, i, (mut,))[2]["state"]
        seg = _TOUCHED.get(mut, slice(None))
        bad = T.ratio(states[i][seg], tuple(v[seg] for v in st))[0]
        print(f"{mut} {c.name} step {i}: good {good:.3f}, mutated {bad:.3e}")
        assert good <= 1.0 and bad > FLOOR, (mut, c.name, i, good, bad)
        worst = min(worst, bad)
    print(f"{mut}: smallest factor {worst:.3e}")


# For the record (asserted is FLOOR): the smallest err / bound each mutation reaches over its steps, rounded down.
MUTATION_FACTORS = {"eps_unclamped": 7.3e4, "handover_older": 1.0e5, "handover_same": 7.8e5, "handover_first": 1.2e6, "noise_neighbour": 3.7e6,
                    "san_c_swap": 5.0e4, "last_not_x0": 2.2e8, "pair_index": 3.1e5, "slot": 5.0e5, "coef_1": 4.3e4,
                    "score_sign": 2.3e5, "ss_std_swap": 2.1e6, "noise_next": 3.3e6, "unscaled_above": 1.4e5, "scaled_below": 2.1e5}


# ------------------------------------------------------------------ reference data for the objectives
OBJECTIVE_CASES = {f"{obj}_eta{eta}": (obj, eta) for obj in ("pred_x0", "pred_v") for eta in (0.0, 0.5)}
GOLD_SHAPE = (24, 4, 20, 3, 6)            # horizon, Lc, R, K, S of ``default``; B = 5, F = 8


@pytest.mark.parametrize("tag", sorted(OBJECTIVE_CASES))
def test_restatement_reproduces_objective_golden(gold_dir, tag):
    obj, eta = OBJECTIVE_CASES[tag]
    hz, Lc, Rr, K, S = GOLD_SHAPE
    g = np.load(os.path.join(gold_dir, "time_compose_objectives.npz"))
    v = {k: torch.from_numpy(g[f"{tag}.{k}"]) for k in ("cond", "init", "step", "img", "img_infered", "states")}
    assert tuple(v["init"].shape) == (K, 5, Rr, 8) and tuple(v["states"].shape) == (S, K, 5, Rr, 8)
    od = O.Diffusion1D(O.synth_state_dict(O.unet1d_param_shapes(hz, 8), seed=0), image_size=Rr, conditioned_steps=Lc, objective=obj)
    states = restated_loop(od, v["cond"], v["init"], v["step"], S, eta)
    for i in range(S):
        scale = float(v["states"][i].abs().max())
        assert float((states[i] - v["states"][i]).abs().max()) <= 2e-6 * scale, (tag, i)
    assert float(g[f"{tag}.clamp_share_min"]) >= 0.005
    assert torch.equal(v["states"][-1][0], v["img"])


# ------------------------------------------------------------------ Langevin
_ULA = {}


def ula_oracle(t, B, L, frozen=False):
    """(x, nz, out, E, U, rows): restated_step_ula of the fp32 oracle with its U-Nets' outputs of the FIRST iteration."""
    key = (t, B, L, frozen)
    if key not in _ULA:
        x, nz = T.ula_inputs(t, B, L)
        od = O.Diffusion1D(_sd(T.ULA_HZ, 8, frozen), image_size=20, conditioned_steps=4, sd_uncond=_sd(T.ULA_HZ, 4, frozen))
        pair, single = _recorded(od)
        b = linear_beta_schedule(T.ULA_N)
        out = restated_step_ula(od, x, t, L, b, scalar_for_gradient(b), nz)
        assert len(pair) == L and len(single) == 4 * L
        if frozen:
            assert all(torch.equal(p, pair[0]) for p in pair) and all(torch.equal(single[k], single[k % 4]) for k in range(4 * L))
        E, U = pair[0].reshape(1, 6, B, T.ULA_HZ, 8), torch.stack(single[:4]).reshape(4, B, T.ULA_HZ, 4)
        _ULA[key] = (x, nz, out, E, U, ula_schedule(b))
    return _ULA[key]


ULA_TAB = O.make_schedule("cosine", 1000, "pred_noise")
ULA_GRID = [(t, B, 1, False) for t in T.ULA_T + T.ULA_T_LOW for B in T.ULA_B] + [(t, 5, 2, True) for t in (401, 999, 400)]


def test_ula_oracle_within_bound():
    for t, B, L, frozen in ULA_GRID:
        x, nz, out, E, U, rows = ula_oracle(t, B, L, frozen)
        st = T.ula_statement(x, nz, t, E, U, ULA_TAB, rows, L)
        r = T.ratio(out, st)[0]
        print(f"ula t{t} B{B} L{L}: err/bound {r:.4f}, n_e {float(st[2].max()):.0f}")
        assert r <= 1.0, (t, B, L, r)
        assert float(st[2].max()) == (5 + (2 if t > 400 else 1) + 2) + 2 * (L - 1)


ULA_MUTATIONS = ("score_sign", "ss_std_swap", "noise_next", "unscaled_above", "scaled_below")


@pytest.mark.parametrize("mut", ULA_MUTATIONS)
def test_ula_mutation_leaves_the_bound(mut):
    ts = {"unscaled_above": (401, 999), "scaled_below": (400, 0)}.get(mut, (401, 731, 400))
    for t in ts:
        x, nz, out, E, U, rows = ula_oracle(t, 5, 1)
        kw, nz_bad = {}, nz
        if mut in ("score_sign", "ss_std_swap"):
            kw["mut"] = (mut,)
        elif mut == "noise_next":
            two = T.ula_inputs(t, 5, 2)[1]
            assert torch.equal(two[0], nz[0])
            nz_bad = two[1:]
        else:
            kw["scaled"] = mut == "scaled_below"
        good = T.ratio(out, T.ula_statement(x, nz, t, E, U, ULA_TAB, rows))[0]
        bad = T.ratio(out, T.ula_statement(x, nz_bad, t, E, U, ULA_TAB, rows, **kw))[0]
        print(f"{mut} t{t}: good {good:.3f}, mutated {bad:.3e}")
        assert good <= 1.0 and bad > FLOOR, (mut, t, good, bad)


def _dec_round_ok(v32, exact):
    """v32 (an fp32 value) is the correctly rounded ``exact`` (Decimal): no neighbour is closer."""
    v = np.float32(v32)
    d = abs(decimal.Decimal(float(v)) - exact)
    return all(d <= abs(decimal.Decimal(float(np.nextafter(v, np.float32(w)))) - exact) for w in (np.inf, -np.inf))


def test_ula_tables_are_correctly_rounded():
    """fp32(float64 formula) == ula_schedule bit for bit, and that value is the correctly rounded exact one: the float64 evaluation is
    within 1e-13 relative of the exact expression (a cumulative product of 1000 factors), 2^-24 / 1e-13 away from moving an fp32
    rounding unless the exact value lies that close to a tie -- none of the 3000 entries does."""
    b = linear_beta_schedule(T.ULA_N)
    sc, ss, sd = ula_schedule(b)
    r64 = R.ula_rows_f64(b)
    for got, want in zip((sc, ss, sd), r64):
        assert want.dtype == torch.float64 and torch.equal(got, want.to(torch.float32))
    decimal.getcontext().prec = 50
    D = decimal.Decimal
    abar = D(1)
    for i in range(T.ULA_N):
        beta = D(float(b[i]))
        abar *= 1 - beta
        step = beta * D(0.035)
        assert _dec_round_ok(float(sc[i]), (1 / (1 - abar)).sqrt()), i
        assert _dec_round_ok(float(ss[i]), step), i
        assert _dec_round_ok(float(sd[i]), (2 * step).sqrt()), i


# ------------------------------------------------------------------ seg_magic
def test_seg_magic_divides_every_admitted_row():
    """floor(row / B) == (row * ceil(2^32 / B)) >> 32 at row = q B - 1 and q B for every B in 1 .. 65535 and every such row below
    65536: the two rows of each multiple at which a wrong quotient would show first."""
    Bs = np.arange(1, 65536, dtype=np.uint64)
    counts = (65536 // Bs).astype(np.int64)                       # q = 1 .. 65536 // B: q B - 1 < 65536
    B = np.repeat(Bs, counts)
    q = (np.arange(B.size, dtype=np.int64) - np.repeat(np.cumsum(counts) - counts, counts) + 1).astype(np.uint64)
    magic = ((np.uint64(1) << np.uint64(32)) + B - np.uint64(1)) // B
    total = 0
    for off in (1, 0):
        rows = q * B - np.uint64(off)
        ok = rows < 65536
        got = (rows * magic) >> np.uint64(32)
        bad = ok & (got != rows // B)
        assert not bool(bad.any()), (int(B[bad][0]), int(rows[bad][0]))
        total += int(ok.sum())
    assert int(magic[0]) == 1 << 32 and total > 1_400_000, total


def test_roundings_by_hand():
    one = torch.ones((1, 4, 16), dtype=torch.float64)
    st = R.ula_update_f64(one, one, one, 5, torch.tensor(2.0), torch.tensor(0.5), torch.tensor(0.25), one)
    assert float(st[0].max()) == 1 - 2 * 0.5 + 0.25 and float(st[1].max()) == 1 + 1 + 0.25 and float(st[2].max()) == 9
    st = R.ula_update_f64(one, one, one, 5, None, torch.tensor(0.5), torch.tensor(0.25), one, A_x=one, n_x=9)
    assert float(st[0].max()) == 1.75 and float(st[2].max()) == 11
    e, A, n = R.rederive_eps_f64(ULA_TAB, 500, one, one, one, 3)
    assert n == 6 and bool((A >= e.abs()).all())
    assert R.BOUND_SLACK == 4
