"""The grid of the parallel time composition and of the Langevin update, shared by tests/test_timecompose_f64_host.py (the fp32
oracle against the float64 statement) and tests/test_gpu_timecompose_f64.py (the library against it).  No GPU and no library call in
here: conditions, tapes, tables and the list of cases.

Time composition.  A case is ONE chain (K segments of B designs, S steps); every step of it is a single-step case of the statement,
because the state before step i is the chain's own record.  Shapes are the smallest that reach every branch of
``timecompose_update_kernel`` (one thread per four features, 256 threads per block):

  horizon 24 = Lc 4 + R 20, F = 8     (K, B) = (3, 5): 600 threads, the ``i >= B * per`` guard falls inside the third block;
                                      (2, 1): one design, the magic division with B = 1; (4, 7): 1120 threads, B no power of two;
                                      (2, 16): 1280 threads, a whole number of blocks
  horizon 8, Lc = R = 4               every row of a segment is handed over
  F = 16, model_unconditioned         the ``multibody`` prediction (six pairs, four single-body rows, uncond_coef 1.4), K = 2, B = 3
  timesteps = sampling_timesteps = 8  the whole chain, with the pairs (1, 0) and (0, -1); see SMALL_T below

each under pred_noise / pred_x0 / pred_v, the clamp on and off, eta 0 and 0.5 (the side cases: both etas, clamp on; multibody: both clamps).

SMALL_T = 8: the fp32 oracle holds the bound at every step of the 8-step cosine schedule (largest ratio 0.27, in the host file's
docstring).  alphas_cumprod runs 3.75e-5 (t = 7: the clipped beta of 0.999, sqrt_recipm1 = 163) .. 0.958 (t = 0); the pair (1, 0)
has 1 - ac/acp = 0.042 at t = 0 under the square root of sigma, and the pair (0, -1) returns x_start.

Langevin.  ``sample_step_ULA`` at one timestep, B in {1, 5}, t in {401, 731, 999} and, below the reference's threshold, {400, 0};
N = 1000, state [B, 24, 16]; the two-iteration cases run on models whose output does not depend on their input."""
import torch

import f64_reference as R

OBJECTIVES = ("pred_noise", "pred_x0", "pred_v")
SMALL_T = 8
SEED = 5301
KB = ((3, 5), (2, 1), (4, 7), (2, 16))


class TCase:
    def __init__(self, index, kind, hz, Lc, K, B, F, objective, clip, eta, T=1000, S=10):
        self.index, self.kind, self.hz, self.Lc, self.R, self.K, self.B, self.F = index, kind, hz, Lc, hz - Lc, K, B, F
        self.objective, self.clip, self.eta, self.T, self.S = objective, clip, eta, T, S
        self.multibody = kind == "multibody"

    @property
    def name(self):
        return f"{self.kind}-K{self.K}B{self.B}-{self.objective}-clip{int(self.clip)}-eta{self.eta}"

    def desc(self):
        return R.ComposeCase("multibody" if self.multibody else "plain", self.F // 4, 1, 0, self.hz, self.Lc, self.objective, self.clip, 1.4)

    def times(self):
        """[(time, time_next)] of the chain."""
        times = list(reversed(torch.linspace(-1, self.T - 1, steps=self.S + 1).int().tolist()))
        return list(zip(times[:-1], times[1:]))


def _cases():
    out = []
    add = lambda *a, **k: out.append(TCase(len(out), *a, **k))
    for obj in OBJECTIVES:
        for clip in (True, False):
            for eta in (0.0, 0.5):
                for K, B in KB:
                    add("grid", 24, 4, K, B, 8, obj, clip, eta)
        for eta in (0.0, 0.5):
            add("whole", 8, 4, 4, 5, 8, obj, True, eta)
            add("small", 24, 4, 3, 5, 8, obj, True, eta, T=SMALL_T, S=SMALL_T)
        for clip in (True, False):
            add("multibody", 24, 4, 2, 3, 16, obj, clip, 0.5)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
GROUPS = sorted({(c.kind, c.objective) for c in CASES})

_INPUTS = {}


def inputs(case):
    """{"cond" [B, Lc, F] (rand - 0.5), "init" [K, B, R, F], "step" [S, K, B, R, F]}: the condition and the tapes of a case."""
    if case.index not in _INPUTS:
        g = torch.Generator().manual_seed(SEED + case.index)
        shape = (case.K, case.B, case.R, case.F)
        _INPUTS[case.index] = {"cond": torch.rand((case.B, case.Lc, case.F), generator=g) - 0.5, "init": torch.randn(shape, generator=g),
                               "step": torch.randn((case.S,) + shape, generator=g)}
    return _INPUTS[case.index]


def state_before(case, d, states, i):
    """The state step i starts from: the init tape, or the record of step i - 1."""
    return d["init"] if i == 0 else states[i - 1]


def statement(case, d, states, i, E, U, tab, row, mut=None):
    """``R.timecompose_step_f64`` of step i of a case: ``states`` [S, K, B, R, F] the chain's own record (step i reads i - 1, the
    ``handover_older`` mutation i - 2), ``E`` / ``U`` the U-Net outputs on ``unet_rows(case, d, states, i)``."""
    t, tn = case.times()[i]
    older = d["init"] if i <= 1 else states[i - 2]
    return R.timecompose_step_f64(tab, case.desc(), state_before(case, d, states, i), d["cond"], t, tn, row, d["step"][i], E, U,
                                  _mut=mut, x_older=older)


def unet_rows(case, d, states, i, mut=None):
    """(pair_in, single_in | None): the rows the U-Nets see at step i (``R.compose_rows`` of cat(hand-over, state)).  The hand-over
    enters a step through these rows alone: its mutations (``R.timecompose_handover``) are made here, and the statement is then
    evaluated on the U-Net outputs of the mutated rows."""
    x = state_before(case, d, states, i)
    older = d["init"] if i <= 1 else states[i - 2]
    c = R.timecompose_handover(x, d["cond"], case.Lc, mut, older).float()
    return R.compose_rows(case.desc(), x.reshape(case.K * case.B, case.R, case.F), c)


def shape_outputs(case, E, U):
    """The U-Nets' outputs in compose_predict_f64's layout: [1, 1, K B, hz, F] (plain) or [1, 6, K B, hz, 8] and [4, K B, hz, 4]."""
    rows = case.K * case.B
    if not case.multibody:
        return E.reshape(1, 1, rows, case.hz, case.F), None
    return E.reshape(1, 6, rows, case.hz, 8), U.reshape(4, rows, case.hz, 4)


def ratio(got, st):
    """(largest |got - ref| / ((n_e + 4) 2^-24 A_e), its index); an element that is exact on both sides counts 0."""
    ref, A, n = st
    got = got.detach().cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), (tuple(got.shape), tuple(ref.shape))
    err = (got.double() - ref).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / R.step1d_bound(n, A))
    i = int(q.argmax())
    return float(q.flatten()[i]), [int(v) for v in torch.unravel_index(torch.tensor(i), q.shape)]


def clamp_share(st):
    return float((st["x_start"][0].abs() == 1.0).double().mean())


# ------------------------------------------------------------------ Langevin
ULA_N, ULA_HZ, ULA_F = 1000, 24, 16
ULA_T = (401, 731, 999)
ULA_T_LOW = (400, 0)
ULA_B = (1, 5)
ULA_DESC = R.ComposeCase("multibody", 4, 1, 0, ULA_HZ, 0, "pred_noise", False, 1.4)


def ula_inputs(t, B, L):
    """(x [B, 24, 16] normal x 0.7, noise [L, B, 24, 16])."""
    g = torch.Generator().manual_seed(SEED + 100 * t + B)
    return torch.randn((B, ULA_HZ, ULA_F), generator=g) * 0.7, torch.randn((L, B, ULA_HZ, ULA_F), generator=g)


def ula_statement(x, nz, t, E, U, tab, rows, L=1, mut=None, scaled=None):
    """``R.ula_update_f64`` over L iterations at timestep t; ``rows`` = the fp32 (scalar, ss, std) tables.  More than one iteration: E
    and U are the same in each (models whose output ignores the input), the state of iteration l is the computed state of l - 1.
    ``scaled``: whether the score carries -scalar[t] (default: the reference's t > 400)."""
    eps, A = R.compose_predict_f64(tab, ULA_DESC, x, None, t, E.double(), U.double())[2:]
    n_eps = R.compose_roundings("multibody", 4, torch.ones(()), "pred_noise")["pred_noise"]
    scaled = t > 400 if scaled is None else scaled
    st = (x.double(), None, 0)
    for l in range(L):
        st = R.ula_update_f64(st[0], eps, A["pred_noise"], n_eps, rows[0][t] if scaled else None, rows[1][t], rows[2][t], nz[l],
                              A_x=st[1], n_x=st[2], _mut=mut)
    return st
