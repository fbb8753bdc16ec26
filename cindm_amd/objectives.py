"""Design objectives.  ``PointObjective`` is the paper's objective for the n-body inverse-design task
(``get_design_fn`` in inference/inverse_design_diffusion_1d.py:211-229 of the reference): drive the last
``last_n_step`` positions of every body to ``pos_target``.

It is an ordinary ``design_fn`` callable (``Tensor[B, L, 4*n_bodies] -> scalar``), so it works on every guided
path; in addition ``GaussianDiffusion1D`` recognises it and, for "standard" / "standard-alpha" guidance (with or
without ``-recurrence-N``), evaluates its closed-form gradient inside the library's update kernel so that the whole
guided reverse loop stays one captured-graph replay (``cindm_ddpm1d_sample_guided``) -- no autograd, no host code in
the loop.  With ``sampling_timesteps < timesteps`` and a ``-recurrence-N`` guidance (N >= 1) the guided DDIM loop is one
library chain in the same way (``cindm_ddpm1d_sample_ddim_guided``).

``WaypointObjective`` is the table form of the same two norms: a target per (design | all designs, row, body) and a non-negative
weight per (design | all designs, row, body).  It covers what the point objective cannot say -- a target per body, a waypoint at an
intermediate row, a sweep of targets and coefficients over the designs of one batch (the reference script loops over such a sweep
call by call, :283-315) -- and takes the same two library chains: the update kernel reads the two tables from device memory
(``cindm_ddpm1d_set_design_tables``, descriptor modes 3 / 4).

``QuadraticObjective`` is the table form of everything that is linear-quadratic in the features of one row: a symmetric ``S`` and a
vector ``h`` per (design | all designs, row), value ``1/2 x^T S x - h^T x`` summed over rows and designs.  A velocity at the end
("arrive and stop"), a relation between bodies ("0 and 1 meet", "keep 2 and 3 apart" with a negative weight), the centre of mass or the
total momentum at a row and any weighted least-squares mix of these are such tables (``from_residuals`` builds them from residuals
``a^T x - r``).  Its gradient acts on all four components of a body -- the first built-in objective whose does -- and takes the same
two library chains (``cindm_ddpm1d_set_design_quadratic``, descriptor mode 5: the guided update compiled with this gradient).

``PairDistanceObjective`` states a relation between the positions of two bodies that is not quadratic: a band ``[lo, hi]`` for the
distance of every (design | all designs, row, pair) with a weight, penalised quadratically outside the band.  "Stay at least d apart"
(``apart``), "come within d" (``within``) and "meet at distance d" (``at``) are such bands and mix freely in one table; the first and
the last are non-convex.  It takes the same two library chains (``cindm_ddpm1d_set_design_pairdist``, descriptor mode 6).

``SumObjective`` is the conjunction of these: at most one waypoint (or point), one quadratic and one pair-distance objective, added.
``a + b`` builds it and ``w * a`` folds a weight into a term's tables.  It takes the same two library chains with every term's tables
armed at once (descriptor mode 7: the guided update evaluates each term as its own kernel does and adds them in the order quadratic,
waypoint, pair-distance)."""
import copy
import math

import torch

from . import _ffi


def _parse_guidance(design_guidance):
    """(alpha, recurrence) of a guidance the library's guided chains evaluate -- "standard" / "standard-alpha", optionally with
    ``-recurrence-N``, N >= 1 an integer -- or None when it needs the generic (autograd) path."""
    g, rec = design_guidance, 0
    if "recurrence" in g:
        try:
            rec = int(g.split("-")[-1])
        except ValueError:
            return None
        g = g[:g.index("-recurrence")]
        if rec < 1:
            return None
    if g not in ("standard", "standard-alpha"):
        return None
    return int(g == "standard-alpha"), rec


def _check_multiple(w, cls, any_sign=False):
    """fp32(w) of a scalar multiple ``w * objective``: finite, and >= 0 unless the objective's tables may carry either sign."""
    if isinstance(w, bool) or not isinstance(w, (int, float)):
        raise TypeError(f"{cls}: a scalar multiple is a real number, not {type(w).__name__}")
    if not math.isfinite(w) or (w < 0 and not any_sign):
        raise ValueError(f"{cls}: the multiple must be finite" + ("" if any_sign else " and >= 0 (its weights are >= 0 by contract)") + f", not {w}")
    return torch.tensor(float(w), dtype=torch.float32)


def _scaled_table(w32, table, cls, name):
    out = w32 * table          # (one fp32 product per entry)
    if not bool(torch.isfinite(out).all()):
        raise ValueError(f"{cls}: the multiple overflows {name}")
    return out.contiguous()


class _Summable:
    """``a + b`` of two built-in objectives is their SumObjective; ``w * a`` is ``a`` with w folded into its tables (``_scaled``)."""

    def __add__(self, other):
        return SumObjective(self, other)

    def __radd__(self, other):
        return SumObjective(other, self)

    def __mul__(self, w):
        return self._scaled(w)

    __rmul__ = __mul__


class PointObjective(_Summable):
    def _scaled(self, w):
        w32 = _check_multiple(w, "PointObjective")
        o = copy.copy(self)
        o.coef = float(w32 * torch.tensor(self.coef, dtype=torch.float32))
        if not math.isfinite(o.coef):
            raise ValueError("PointObjective: the multiple overflows coef")
        o.time_consistency_coef = float(w) * self.time_consistency_coef
        return o

    def __init__(self, pos_target, last_n_step, gamma=2, coef=100, time_consistency_coef=0, design_fn_mode="L2"):
        pos_target = torch.as_tensor(pos_target, dtype=torch.float32).reshape(-1)
        assert pos_target.numel() == 2, "pos_target is a 2-D position"
        assert gamma == 2, "the reference asserts gamma == 2"
        if design_fn_mode not in ("L2", "L2square"):
            raise ValueError(design_fn_mode)
        self.pos_target, self.last_n_step, self.gamma = pos_target, int(last_n_step), gamma
        self.coef, self.time_consistency_coef, self.design_fn_mode = float(coef), float(time_consistency_coef), design_fn_mode

    def __call__(self, pos):
        """pos: [B, steps, n_bodies*4] -> scalar loss (summed over the batch, as the reference does)."""
        n_bodies = pos.shape[-1] // 4
        target = self.pos_target.to(pos.device)
        n = self.last_n_step
        per_body = []
        for jj in range(n_bodies):
            sq = ((pos[..., -n:, jj * 4:jj * 4 + 2] - target).abs() ** 2).sum(-1)
            if self.design_fn_mode == "L2":
                sq = sq ** 0.5
            per_body.append(sq.mean(-1).sum(0))
        total = torch.stack(per_body).sum() * self.coef
        if self.time_consistency_coef > 0:
            idx = torch.cat([torch.arange(ii * 4, ii * 4 + 2) for ii in range(n_bodies)]).to(pos.device)
            total = total + (pos[:, 1:, idx] - pos[:, :-1, idx]).square().sum(-1).mean(-1).sum() * self.time_consistency_coef
        return total

    def descriptor(self, design_guidance):
        """cindm_design_desc for this objective under ``design_guidance``, or None when that guidance needs the generic
        (autograd) path."""
        parsed = _parse_guidance(design_guidance)
        if parsed is None:
            return None
        d = _ffi.DesignDesc()
        d.mode = 1 if self.design_fn_mode == "L2" else 2
        d.alpha, d.recurrence = parsed
        d.last_n_step = self.last_n_step
        d.coef, d.time_consistency_coef = self.coef, self.time_consistency_coef
        d.pos_target[0], d.pos_target[1] = float(self.pos_target[0]), float(self.pos_target[1])
        return d


class _TableObjective(_Summable):
    """What the table objectives share.  A subclass declares ``_TABLES``, its table attributes with the rank each has when it is
    shared by every design (one more: per design); ``_WIDTH``, the attribute that counts what a row of its tables holds, the noun
    for it and how many a body has; ``_SETTER``, the library entry that arms its two device tables; ``mode``, its descriptor mode.
    ``rows`` and the width attribute are the subclass's own."""
    _TABLES, _WIDTH, _SETTER = (), ("n_bodies", "bodies", 1), ""
    _SCALED, _ANY_SIGN = (), False          # the tables a scalar multiple scales; whether it may be negative

    def _scaled(self, w):
        """``w * self``: a copy with fp32(w) folded into the ``_SCALED`` tables (one fp32 product per entry) and w into the
        time-consistency coefficient.  The kernels have no per-term weight."""
        cls = type(self).__name__
        w32 = _check_multiple(w, cls, self._ANY_SIGN)
        if w < 0 and self.time_consistency_coef != 0:
            raise ValueError(f"{cls}: a negative multiple of an objective with a time-consistency term (the kernels apply that term for a coefficient > 0 only)")
        o = copy.copy(self)
        for name in self._SCALED:
            setattr(o, name, _scaled_table(w32, getattr(self, name), cls, name))
        o.time_consistency_coef = float(w) * self.time_consistency_coef
        o._dev = {}
        return o

    def _without_time_consistency(self):
        o = copy.copy(self)
        o.time_consistency_coef = 0.0
        return o

    @property
    def per_design(self):
        """Designs the per-design tables are for, or None when all tables are shared by every design."""
        for name, rank in self._TABLES:
            v = getattr(self, name)
            if v.dim() == rank + 1:
                return v.shape[0]
        return None

    def check_state(self, B, L, n_bodies):
        """ValueError unless the tables fit a state [B, L, 4 * n_bodies]."""
        cls = type(self).__name__
        attr, noun, per_body = self._WIDTH
        if self.rows != L:
            raise ValueError(f"{cls}: tables of {self.rows} rows, the state has {L}")
        if getattr(self, attr) != per_body * n_bodies:
            raise ValueError(f"{cls}: tables of {getattr(self, attr)} {noun}, the state has {per_body * n_bodies}")
        if self.per_design is not None and self.per_design != B:
            raise ValueError(f"{cls}: per-design tables for {self.per_design} designs, the batch has {B} "
                             "(shard(lo, hi) slices them for a part of the batch)")

    def shard(self, lo, hi):
        """The objective of designs lo .. hi-1: per-design tables sliced, tables shared by every design passed through."""
        o = copy.copy(self)
        for name, rank in self._TABLES:
            v = getattr(self, name)
            setattr(o, name, v[lo:hi].contiguous() if v.dim() == rank + 1 else v)
        o._dev = {}
        return o

    def _host_tables(self):
        """The two tables the kernel reads, on the CPU: [L, ..] or [B, L, ..] each."""
        return tuple(getattr(self, name) for name, _ in self._TABLES)

    def tables(self, device):
        """The two contiguous fp32 tensors on ``device`` (cached per device) the kernel reads."""
        device = torch.device(device)
        if device not in self._dev:
            self._dev[device] = tuple(v.to(device).contiguous() for v in self._host_tables())
        return self._dev[device]

    def _time_consistency(self, pos, n_bodies):
        idx = torch.cat([torch.arange(ii * 4, ii * 4 + 2) for ii in range(n_bodies)]).to(pos.device)
        return (pos[:, 1:, idx] - pos[:, :-1, idx]).square().sum(-1).mean(-1).sum() * self.time_consistency_coef

    def _time_consistency_grad(self, x):
        """The time-consistency term of ``closed_form_grad`` on the positions x [B, L, nb, 2], L > 1, as the kernels evaluate it:
        ((tc * 2) * lap) / (L - 1),  lap = (x_l - x_{l-1}) [l >= 1] - (x_{l+1} - x_l) [l + 1 < L]."""
        lap = torch.zeros_like(x)
        lap[:, 1:] += x[:, 1:] - x[:, :-1]
        lap[:, :-1] -= x[:, 1:] - x[:, :-1]
        return self.time_consistency_coef * 2.0 * lap / float(x.shape[1] - 1)

    def descriptor(self, design_guidance):
        """cindm_design_desc (the tables are armed per call) for this objective under ``design_guidance``, or None when that
        guidance needs the generic (autograd) path."""
        parsed = _parse_guidance(design_guidance)
        if parsed is None:
            return None
        d = _ffi.DesignDesc()
        d.mode = self.mode
        d.alpha, d.recurrence = parsed
        d.time_consistency_coef = self.time_consistency_coef
        return d

    def arm(self, handle, B, device):
        """Arms the next guided chain call on ``handle`` (a cindm_ddpm1d) with this objective's tables, for a batch of ``B`` designs
        (per-design tables declare their own extent: the chain call refuses another batch)."""
        a, b = self.tables(device)          # [B | -, L, .., ..] and [B | -, L, ..]
        batch = B if self.per_design is None else self.per_design
        _ffi.check(getattr(_ffi.lib(), self._SETTER)(handle, _ffi.ptr(a), int(a.dim() == 4), _ffi.ptr(b), int(b.dim() == 3),
                                                     self.rows, getattr(self, self._WIDTH[0]), batch))


class WaypointObjective(_TableObjective):
    """``target`` [L, nb, 2] or [B, L, nb, 2]: the position (features 4j, 4j+1) body j is drawn to at that row, in state units.
    ``weight`` [L, nb] or [B, L, nb]: finite, >= 0; 0 = no waypoint at that (row, body).  The value for pos [B, L, 4*nb] is

        sum_b sum_l sum_j scale[b, l, j] * ||pos[b, l, 4j:4j+2] - target[b, l, j]||_2          ("L2"; squared for "L2square")
        + the time-consistency term of PointObjective

    with scale = fp32(coef) * fp32(weight), formed once: ``__call__`` and the kernel read the same table.  An entry whose scale is 0
    contributes exactly 0 to the value and to the gradient, also where pos == target."""

    def __init__(self, target, weight, *, coef=1.0, time_consistency_coef=0.0, design_fn_mode="L2", _scale=None):
        """``_scale``: a ready fp32 scale table in place of coef * weight (from_point's, formed by a division)."""
        if design_fn_mode not in ("L2", "L2square"):
            raise ValueError(design_fn_mode)
        if _scale is None:
            weight = torch.as_tensor(weight).detach().to("cpu", torch.float32)
            if not bool(torch.isfinite(weight).all()) or bool((weight < 0).any()):
                raise ValueError("weight must be finite and >= 0")
            _scale = torch.tensor(float(coef), dtype=torch.float32) * weight
        target = torch.as_tensor(target).detach().to("cpu", torch.float32).contiguous()
        scale = torch.as_tensor(_scale).detach().to("cpu", torch.float32).contiguous()
        if target.dim() not in (3, 4) or target.shape[-1] != 2:
            raise ValueError(f"target must be [L, nb, 2] or [B, L, nb, 2], not {tuple(target.shape)}")
        if scale.dim() not in (2, 3):
            raise ValueError(f"weight must be [L, nb] or [B, L, nb], not {tuple(scale.shape)}")
        if tuple(target.shape[-3:-1]) != tuple(scale.shape[-2:]) or 0 in target.shape or 0 in scale.shape:
            raise ValueError(f"target {tuple(target.shape)} and weight {tuple(scale.shape)} disagree on (L, nb)")
        if target.dim() == 4 and scale.dim() == 3 and target.shape[0] != scale.shape[0]:
            raise ValueError(f"target is for {target.shape[0]} designs, weight for {scale.shape[0]}")
        if not bool(torch.isfinite(target).all()):
            raise ValueError("target must be finite")
        if not bool(torch.isfinite(scale).all()) or bool((scale < 0).any()):
            raise ValueError("coef * weight must be finite and >= 0")
        self.target, self.scale = target, scale
        self.time_consistency_coef, self.design_fn_mode = float(time_consistency_coef), design_fn_mode
        self._dev = {}

    @classmethod
    def from_point(cls, pos_target, last_n_step, L, n_bodies, coef=100, time_consistency_coef=0, design_fn_mode="L2"):
        """The table form of ``PointObjective(pos_target, last_n_step, coef=coef, ...)`` on a state of ``L`` rows and ``n_bodies``
        bodies: scale = fp32(coef) / fp32(last_n_step) -- the one division the kernel's point branch does -- on the last n rows."""
        n, L, nb = int(last_n_step), int(L), int(n_bodies)
        if not 1 <= n <= L:
            raise ValueError(f"last_n_step {n} outside 1 .. L = {L}")
        pt = torch.as_tensor(pos_target, dtype=torch.float32).reshape(-1)
        if pt.numel() != 2:
            raise ValueError("pos_target is a 2-D position")
        scale = torch.zeros((L, nb), dtype=torch.float32)
        scale[L - n:] = torch.tensor(float(coef), dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)
        return cls(pt.expand(L, nb, 2), None, time_consistency_coef=time_consistency_coef, design_fn_mode=design_fn_mode, _scale=scale)

    # ------------------------------------------------------------------ shapes
    _TABLES, _SETTER, _SCALED = (("target", 3), ("scale", 2)), "cindm_ddpm1d_set_design_tables", ("scale",)

    @property
    def mode(self):
        return 3 if self.design_fn_mode == "L2" else 4

    @property
    def rows(self):
        return self.scale.shape[-2]

    @property
    def n_bodies(self):
        return self.scale.shape[-1]

    # ------------------------------------------------------------------ value and gradient
    def __call__(self, pos):
        """pos: [B, L, n_bodies*4] -> scalar loss (summed over the batch)."""
        B, L, F = pos.shape
        self.check_state(B, L, F // 4)
        target, scale = self.target.to(pos), self.scale.to(pos)
        on = scale > 0
        sq = (pos.reshape(B, L, F // 4, 4)[..., :2] - target).square().sum(-1)
        if self.design_fn_mode == "L2":
            # (the square root only sees entries that count: its derivative at 0 is inf, and 0 * inf would reach the gradient)
            sq = torch.sqrt(torch.where(on, sq, torch.ones_like(sq)))
        total = torch.where(on, scale * sq, torch.zeros_like(sq)).sum()
        if self.time_consistency_coef > 0:
            total = total + self._time_consistency(pos, F // 4)
        return total

    def closed_form_grad(self, pos):
        """The gradient of ``__call__`` as compose_update_element evaluates it, operation for operation (the kernel's table branch
        followed by its time-consistency term): per position component, d = pos - target,
            "L2": (s * d) / sqrt(d * d + d_other * d_other),   "L2square": (s * 2) * d,   skipped where s == 0,
            + ((tc * 2) * lap) / (L - 1),  lap = (x_l - x_{l-1}) [l >= 1] - (x_{l+1} - x_l) [l + 1 < L]."""
        B, L, F = pos.shape
        self.check_state(B, L, F // 4)
        target, scale = self.target.to(pos), self.scale.to(pos)
        x = pos.reshape(B, L, F // 4, 4)[..., :2]
        s = scale.unsqueeze(-1).expand(x.shape)
        on = s != 0
        d = x - target
        if self.design_fn_mode == "L2":
            dd = d * d
            den = torch.sqrt(torch.where(on, dd + dd.flip(-1), torch.ones_like(dd)))
            g = s * d / den
        else:
            g = s * 2.0 * d
        g = torch.where(on, g, torch.zeros_like(g))
        if self.time_consistency_coef > 0 and L > 1:
            g = g + self._time_consistency_grad(x)
        out = torch.zeros_like(pos).reshape(B, L, F // 4, 4)
        out[..., :2] = g
        return out.reshape(B, L, F)


class QuadraticObjective(_TableObjective):
    """``S`` [L, F, F] or [B, L, F, F]: a symmetric matrix per row (exactly: S[.., f, g] == S[.., g, f]); ``h`` [L, F] or [B, L, F].
    F = 4 * n_bodies, a multiple of 4 up to 32.  The value for pos [B, L, F] is

        sum_b sum_l ( 1/2 pos[b, l]^T S[b | 0, l] pos[b, l] - h[b | 0, l]^T pos[b, l] )  + the time-consistency term of PointObjective

    and its gradient at (b, l, f) is (sum_f' S[l, f, f'] pos[b, l, f']) - h[l, f] on every feature, velocities included (+ the
    time-consistency term on the position features).  S need not be positive: a negative weight pushes away."""

    def __init__(self, S, h, *, time_consistency_coef=0.0):
        S = torch.as_tensor(S).detach().to("cpu", torch.float32).contiguous()
        h = torch.as_tensor(h).detach().to("cpu", torch.float32).contiguous()
        if S.dim() not in (3, 4) or S.shape[-1] != S.shape[-2]:
            raise ValueError(f"S must be [L, F, F] or [B, L, F, F], not {tuple(S.shape)}")
        if h.dim() not in (2, 3):
            raise ValueError(f"h must be [L, F] or [B, L, F], not {tuple(h.shape)}")
        F = S.shape[-1]
        if F < 4 or F % 4 != 0 or F > 32:
            raise ValueError(f"F = {F}: the features of a row are 4 per body, a multiple of 4 in 4 .. 32")
        if tuple(S.shape[-3:-1]) != tuple(h.shape[-2:]) or 0 in S.shape or 0 in h.shape:
            raise ValueError(f"S {tuple(S.shape)} and h {tuple(h.shape)} disagree on (L, F)")
        if S.dim() == 4 and h.dim() == 3 and S.shape[0] != h.shape[0]:
            raise ValueError(f"S is for {S.shape[0]} designs, h for {h.shape[0]}")
        if not bool(torch.isfinite(S).all()) or not bool(torch.isfinite(h).all()):
            raise ValueError("S and h must be finite")
        if not torch.equal(S, S.transpose(-1, -2)):
            raise ValueError("S must be symmetric, exactly (from_residuals builds such tables; or pass (S + S^T) / 2)")
        self.S, self.h = S, h
        self.time_consistency_coef = float(time_consistency_coef)
        self._dev = {}

    @classmethod
    def from_residuals(cls, rows, A, r, weight, L, F, *, time_consistency_coef=0.0):
        """The least-squares form: residual m is ``A[m]^T pos[:, rows[m]] - r[m]`` with weight ``weight[m]`` (any sign), and the value
        is 1/2 sum_m weight[m] residual_m^2 up to its constant 1/2 sum_m weight[m] r[m]^2.  ``rows`` [M] ints in 0 .. L-1; ``A`` [M, F],
        ``r`` [M], ``weight`` [M], each optionally with a leading designs axis B (then the tables it enters are per design).
        S_l = sum w a a^T and h_l = sum w r a are accumulated in float64 and cast to fp32 once: S is exactly symmetric."""
        L, F = int(L), int(F)
        rows = torch.as_tensor(rows, dtype=torch.int64).reshape(-1)
        M = rows.numel()
        A, r, w = (torch.as_tensor(v).detach().to("cpu", torch.float64) for v in (A, r, weight))
        if M and (int(rows.min()) < 0 or int(rows.max()) >= L):
            raise ValueError(f"rows outside 0 .. L - 1 = {L - 1}")
        if A.dim() not in (2, 3) or tuple(A.shape[-2:]) != (M, F):
            raise ValueError(f"A must be [M, F] or [B, M, F] with M = {M}, F = {F}, not {tuple(A.shape)}")
        for name, v in (("r", r), ("weight", w)):
            if v.dim() not in (1, 2) or v.shape[-1] != M:
                raise ValueError(f"{name} must be [M] or [B, M] with M = {M}, not {tuple(v.shape)}")
        nB = {v.shape[0] for v, d in ((A, 3), (r, 2), (w, 2)) if v.dim() == d}
        if len(nB) > 1:
            raise ValueError(f"A, r and weight disagree on the number of designs: {sorted(nB)}")
        B = nB.pop() if nB else None
        lead = lambda *vs: any(v.dim() == d for v, d in vs)
        # (a a^T first: its (f, g) and (g, f) entries are the same product, and both are scaled and summed in the same order)
        wa2 = w[..., None, None] * (A[..., :, None] * A[..., None, :])          # [B |, M, F, F]
        wra = (w * r)[..., None] * A                                            # [B |, M, F]
        if lead((A, 3), (w, 2)):
            S = torch.zeros((B, L, F, F), dtype=torch.float64).index_add_(1, rows, wa2.expand(B, M, F, F))
        else:
            S = torch.zeros((L, F, F), dtype=torch.float64).index_add_(0, rows, wa2)
        if B is not None:
            hh = torch.zeros((B, L, F), dtype=torch.float64).index_add_(1, rows, wra.expand(B, M, F))
        else:
            hh = torch.zeros((L, F), dtype=torch.float64).index_add_(0, rows, wra)
        return cls(S.to(torch.float32), hh.to(torch.float32), time_consistency_coef=time_consistency_coef)

    # ------------------------------------------------------------------ shapes
    _TABLES, _WIDTH, _SETTER, mode = (("S", 3), ("h", 2)), ("features", "features", 4), "cindm_ddpm1d_set_design_quadratic", 5
    _SCALED, _ANY_SIGN = ("S", "h"), True

    @property
    def rows(self):
        return self.h.shape[-2]

    @property
    def features(self):
        return self.h.shape[-1]

    # ------------------------------------------------------------------ value and gradient
    def __call__(self, pos):
        """pos: [B, L, F] -> scalar loss (summed over the batch)."""
        B, L, F = pos.shape
        self.check_state(B, L, F // 4)
        S, h = self.S.to(pos), self.h.to(pos)
        Sx = (S @ pos.unsqueeze(-1)).squeeze(-1)
        total = 0.5 * (pos * Sx).sum() - (h * pos).sum()
        if self.time_consistency_coef > 0 and L > 1:
            total = total + self._time_consistency(pos, F // 4)
        return total

    def closed_form_grad(self, pos):
        """The gradient of ``__call__`` as compose_update_quad_kernel evaluates it, operation for operation: per element (b, l, f)
            acc = 0;  acc = acc + S[l, f, f'] * pos[b, l, f']  for f' = 0 .. F-1 (each product and each sum rounded once);  g = acc - h[l, f];
            on position features  g = g + ((tc * 2) * lap) / (L - 1),  lap = (x_l - x_{l-1}) [l >= 1] - (x_{l+1} - x_l) [l + 1 < L]."""
        B, L, F = pos.shape
        self.check_state(B, L, F // 4)
        S, h = self.S.to(pos), self.h.to(pos)
        acc = torch.zeros_like(pos)
        for fp in range(F):
            acc = acc + S[..., :, fp] * pos[..., fp:fp + 1]
        g = acc - h
        if self.time_consistency_coef > 0 and L > 1:
            x = pos.reshape(B, L, F // 4, 4)[..., :2]
            g = g.reshape(B, L, F // 4, 4).clone()
            g[..., :2] = g[..., :2] + self._time_consistency_grad(x)
            g = g.reshape(B, L, F)
        return g


_PAIR_COUNTS = {nb * (nb - 1) // 2: nb for nb in range(2, 9)}        # P -> n_bodies, 2 .. 8 bodies


def pair_index(i, j, n_bodies):
    """The library's pair order (0,1), (0,2), .., (1,2), ..: the index of pair (i, j), i < j (``pair_index`` in kernels.h)."""
    return i * n_bodies - (i * (i + 1)) // 2 + (j - i - 1)


class PairDistanceObjective(_TableObjective):
    """``lo``, ``hi``, ``weight``: each [L, P] or [B, L, P], P = nb (nb - 1) / 2 pairs (i, j), i < j, in the order of ``pair_index``.
    0 <= lo <= hi, lo finite, hi finite or +inf; weight finite, >= 0 (0 = no relation at that (row, pair)).  With r the distance
    between the positions (features 4i, 4i+1 and 4j, 4j+1) of the pair's bodies, the value for pos [B, L, 4 * nb] is

        sum_b sum_l sum_p weight[b | 0, l, p] * ( max(lo[b | 0, l, p] - r, 0)^2 + max(r - hi[b | 0, l, p], 0)^2 )
        + the time-consistency term of PointObjective

    The penalty is C1 at r = lo and r = hi; its direction is undefined at r = 0, where the gradient is defined as 0: ``__call__`` masks
    coincident pairs ahead of the square root, so autograd gives 0 there and not NaN, and the kernel and ``closed_form_grad`` skip them.

    What the kernel evaluates (``closed_form_grad`` restates it) at position component c of body i, over the other bodies o in
    ascending o from 0.f: d = pos_i,c - pos_o,c; r = sqrt(d * d + d' * d') with d' the other component's difference;
    term = ((((w * 2) * (r - lo)) * d) / r where r < lo, ((((w * 2) * (r - hi)) * d) / r where r > hi, else 0.f, and 0.f where w == 0 or
    r == 0; g = g + term.  Every difference, product, sum, square root and quotient is rounded once, in the order written."""

    def __init__(self, lo, hi, weight, *, time_consistency_coef=0.0):
        lo, hi, weight = (torch.as_tensor(v).detach().to("cpu", torch.float32).contiguous() for v in (lo, hi, weight))
        for name, v in (("lo", lo), ("hi", hi), ("weight", weight)):
            if v.dim() not in (2, 3) or 0 in v.shape:
                raise ValueError(f"{name} must be [L, P] or [B, L, P], not {tuple(v.shape)}")
        if not (tuple(lo.shape[-2:]) == tuple(hi.shape[-2:]) == tuple(weight.shape[-2:])):
            raise ValueError(f"lo {tuple(lo.shape)}, hi {tuple(hi.shape)} and weight {tuple(weight.shape)} disagree on (L, P)")
        nB = {v.shape[0] for v in (lo, hi, weight) if v.dim() == 3}
        if len(nB) > 1:
            raise ValueError(f"lo, hi and weight disagree on the number of designs: {sorted(nB)}")
        P = weight.shape[-1]
        if P not in _PAIR_COUNTS:
            raise ValueError(f"P = {P}: the pairs of 2 .. 8 bodies are {sorted(_PAIR_COUNTS)}")
        if not bool(torch.isfinite(lo).all()) or bool((lo < 0).any()):
            raise ValueError("lo must be finite and >= 0")
        if not bool((hi >= lo).all()):          # (NaN fails the comparison; +inf passes)
            raise ValueError("hi must be >= lo (+inf allowed, NaN not)")
        if not bool(torch.isfinite(weight).all()) or bool((weight < 0).any()):
            raise ValueError("weight must be finite and >= 0")
        self.lo, self.hi, self.weight = lo, hi, weight
        self.time_consistency_coef = float(time_consistency_coef)
        self._dev = {}

    @staticmethod
    def _table(d, weight):
        """``d`` (a number, or a table that broadcasts against weight's [L, P]) as an fp32 table [L, P] or [B, L, P]."""
        weight = torch.as_tensor(weight)
        d = torch.as_tensor(d).detach().to("cpu", torch.float32)
        return d.expand(weight.shape[-2:]).contiguous() if d.dim() < 2 else d

    @classmethod
    def apart(cls, d, weight, *, time_consistency_coef=0.0):
        """The pair stays at least ``d`` apart: the band [d, +inf)."""
        lo = cls._table(d, weight)
        return cls(lo, torch.full_like(lo, float("inf")), weight, time_consistency_coef=time_consistency_coef)

    @classmethod
    def within(cls, d, weight, *, time_consistency_coef=0.0):
        """The pair comes within ``d``: the band [0, d]."""
        hi = cls._table(d, weight)
        return cls(torch.zeros_like(hi), hi, weight, time_consistency_coef=time_consistency_coef)

    @classmethod
    def at(cls, d, weight, *, time_consistency_coef=0.0):
        """The pair meets at distance exactly ``d``: the band [d, d]."""
        lo = cls._table(d, weight)
        return cls(lo, lo.clone(), weight, time_consistency_coef=time_consistency_coef)

    # ------------------------------------------------------------------ shapes
    _TABLES, _SETTER, mode = (("lo", 2), ("hi", 2), ("weight", 2)), "cindm_ddpm1d_set_design_pairdist", 6
    _SCALED = ("weight",)

    @property
    def rows(self):
        return self.weight.shape[-2]

    @property
    def n_bodies(self):
        return _PAIR_COUNTS[self.weight.shape[-1]]

    def _host_tables(self):
        """(band, weight): band [B | -, L, P, 2] holds (lo, hi) interleaved; lo and hi share one per-design flag: where either is per
        design both are materialised."""
        lo, hi = self.lo, self.hi
        if lo.dim() != hi.dim():
            shape = lo.shape if lo.dim() == 3 else hi.shape
            lo, hi = lo.expand(shape), hi.expand(shape)
        return torch.stack((lo, hi), dim=-1), self.weight

    # ------------------------------------------------------------------ value and gradient
    def _pairs(self):
        nb = self.n_bodies
        ij = [(i, j) for i in range(nb) for j in range(i + 1, nb)]
        return torch.tensor([i for i, _ in ij]), torch.tensor([j for _, j in ij])

    def __call__(self, pos):
        """pos: [B, L, n_bodies*4] -> scalar loss (summed over the batch)."""
        B, L, F = pos.shape
        self.check_state(B, L, F // 4)
        lo, hi, w = self.lo.to(pos), self.hi.to(pos), self.weight.to(pos)
        I, J = (v.to(pos.device) for v in self._pairs())
        x = pos.reshape(B, L, F // 4, 4)[..., :2]
        sq = (x[:, :, I] - x[:, :, J]).square().sum(-1)                  # [B, L, P]
        # (the square root only sees pairs that are apart: its derivative at 0 is inf, and 0 * inf would reach the gradient; a
        #  coincident pair has r = 0 as a constant -- the right value, and the zero gradient the kernel defines there)
        apart = sq > 0
        r = torch.where(apart, torch.sqrt(torch.where(apart, sq, torch.ones_like(sq))), torch.zeros_like(sq))
        pen = (lo - r).clamp(min=0).square() + (r - hi).clamp(min=0).square()
        total = torch.where(w > 0, w * pen, torch.zeros_like(pen)).sum()
        if self.time_consistency_coef > 0 and L > 1:
            total = total + self._time_consistency(pos, F // 4)
        return total

    def closed_form_grad(self, pos):
        """The gradient of ``__call__`` as compose_update_pair_kernel evaluates it, operation for operation: per position component c
        of body i, acc = 0; for o = 0 .. nb-1, o != i, with (w, lo, hi) the entry of the pair {i, o}:
            d = pos_i,c - pos_o,c;  r = sqrt(d_x * d_x + d_y * d_y);
            term = ((((w * 2) * (r - lo)) * d) / r  where r < lo,  ((((w * 2) * (r - hi)) * d) / r  where r > hi,  else 0;
            term = 0 where w == 0 or r == 0;  acc = acc + term
        (each operation rounded once in the dtype of ``pos``), then on position features
            g = acc + ((tc * 2) * lap) / (L - 1),  lap = (x_l - x_{l-1}) [l >= 1] - (x_{l+1} - x_l) [l + 1 < L]."""
        B, L, F = pos.shape
        nb = F // 4
        self.check_state(B, L, nb)
        lo, hi, w = (v.to(pos).unsqueeze(-1) for v in (self.lo, self.hi, self.weight))      # [B | -, L, P, 1]
        x = pos.reshape(B, L, nb, 4)[..., :2]
        g = torch.zeros_like(x)
        for i in range(nb):
            acc = torch.zeros_like(x[:, :, i])
            for o in range(nb):
                if o == i:
                    continue
                p = pair_index(min(i, o), max(i, o), nb)
                wp, lop, hip = w[..., p, :], lo[..., p, :], hi[..., p, :]
                d = x[:, :, i] - x[:, :, o]                                               # [B, L, 2]
                dd = d * d
                r = torch.sqrt(dd[..., 0:1] + dd[..., 1:2])
                below = r < lop
                active = (wp != 0) & (r != 0) & (below | (r > hip))
                # (the unselected side may hold inf or NaN -- r - inf, a quotient by 0 -- and is never read)
                bound = torch.where(below, lop, torch.where(active, hip, r))
                term = (((wp * 2.0) * (r - bound)) * d) / torch.where(active, r, torch.ones_like(r))
                acc = acc + torch.where(active, term, torch.zeros_like(term))
            g[:, :, i] = acc
        if self.time_consistency_coef > 0 and L > 1:
            g = g + self._time_consistency_grad(x)
        out = torch.zeros_like(pos).reshape(B, L, nb, 4)
        out[..., :2] = g
        return out.reshape(B, L, F)


_SUM_KINDS = ("quadratic", "waypoint", "pair-distance")          # the order the kernel adds the terms in


def _sum_kind(term):
    if isinstance(term, QuadraticObjective):
        return "quadratic"
    if isinstance(term, (WaypointObjective, PointObjective)):
        return "waypoint"
    if isinstance(term, PairDistanceObjective):
        return "pair-distance"
    raise TypeError(f"SumObjective: a term is a WaypointObjective, QuadraticObjective, PairDistanceObjective or PointObjective, not {type(term).__name__}")


class SumObjective:
    """The sum of built-in objectives: at most one term of each kind -- quadratic, waypoint (a ``PointObjective`` counts as its table
    form, ``WaypointObjective.from_point``, made once the state's (L, n_bodies) are known), pair-distance.  ``a + b`` builds it and adding
    a further term flattens; two terms of a kind are refused (merging tables would change roundings: merge them yourself).  There is no
    per-term weight in the kernel: ``w * term`` folds one into the term's tables.

    The value is the sum of the terms' values in the order quadratic, waypoint, pair-distance; the time-consistency coefficient is the
    sum of the terms' and the kernel applies that term once.  The library's guided chains run it with every term's tables armed
    (descriptor mode 7, compose_update_sum_kernel); a sum of one term is that term, bit for bit."""

    def __init__(self, *terms):
        flat = []
        for t in terms:
            flat.extend(t.terms if isinstance(t, SumObjective) else (t,))
        if not flat:
            raise ValueError("SumObjective: no terms")
        by_kind = {}
        for t in flat:
            kind = _sum_kind(t)
            if kind in by_kind:
                raise ValueError(f"SumObjective: two {kind} terms ({type(by_kind[kind]).__name__} and {type(t).__name__}); a sum holds at most one "
                                 "term of a kind and does not merge tables")
            by_kind[kind] = t
        self.terms = tuple(by_kind[k] for k in _SUM_KINDS if k in by_kind)          # kernel order, whatever the operand order
        self._agree()
        self._tabled, self._last = {}, None

    def _agree(self):
        """ValueError unless the table terms agree on (L, n_bodies) and on the per-design extent."""
        shapes = {(t.rows, getattr(t, t._WIDTH[0]) // t._WIDTH[2]) for t in self.terms if isinstance(t, _TableObjective)}
        if len(shapes) > 1:
            raise ValueError(f"SumObjective: the terms disagree on (L, n_bodies): {sorted(shapes)}")
        extents = {t.per_design for t in self.terms if isinstance(t, _TableObjective) and t.per_design is not None}
        if len(extents) > 1:
            raise ValueError(f"SumObjective: the terms' per-design tables are for different numbers of designs: {sorted(extents)}")

    # ------------------------------------------------------------------ algebra
    def __add__(self, other):
        return SumObjective(self, other)

    def __radd__(self, other):
        return SumObjective(other, self)

    def __mul__(self, w):
        return SumObjective(*(t * w for t in self.terms))

    __rmul__ = __mul__

    # ------------------------------------------------------------------ shapes
    @property
    def time_consistency_coef(self):
        return float(sum(float(t.time_consistency_coef) for t in self.terms))

    @property
    def per_design(self):
        """Designs the terms' per-design tables are for, or None when every table is shared by every design."""
        for t in self.terms:
            if isinstance(t, _TableObjective) and t.per_design is not None:
                return t.per_design
        return None

    def table_terms(self, L, n_bodies):
        """The terms as table objectives on a state of ``L`` rows and ``n_bodies`` bodies, in kernel order: a PointObjective term becomes
        ``WaypointObjective.from_point`` (cached per (L, n_bodies), so its device tables are made once)."""
        key = (int(L), int(n_bodies))
        if key not in self._tabled:
            self._tabled[key] = tuple(
                WaypointObjective.from_point(t.pos_target, t.last_n_step, L, n_bodies, coef=t.coef, time_consistency_coef=t.time_consistency_coef,
                                             design_fn_mode=t.design_fn_mode) if isinstance(t, PointObjective) else t
                for t in self.terms)
        return self._tabled[key]

    def check_state(self, B, L, n_bodies):
        """ValueError unless every term fits a state [B, L, 4 * n_bodies] (each term's own check) and the terms' per-design extents agree."""
        self._agree()
        for t in self.table_terms(L, n_bodies):
            t.check_state(B, L, n_bodies)
        self._last = (int(L), int(n_bodies))

    def shard(self, lo, hi):
        """The objective of designs lo .. hi-1: every term sharded (a PointObjective term has nothing per design)."""
        return type(self)(*(t.shard(lo, hi) if isinstance(t, _TableObjective) else t for t in self.terms))

    # ------------------------------------------------------------------ value and gradient
    def __call__(self, pos):
        """pos: [B, L, n_bodies*4] -> scalar loss (summed over the batch): the terms' values added in kernel order."""
        B, L, F = pos.shape
        self.check_state(B, L, F // 4)
        total = None
        for t in self.table_terms(L, F // 4):
            v = t(pos)
            total = v if total is None else total + v
        return total

    def closed_form_grad(self, pos):
        """The gradient of ``__call__`` as compose_update_sum_kernel evaluates it, operation for operation, in the dtype of ``pos``:
        each term's ``closed_form_grad`` without its time-consistency term; g = the first term's, then g = g + the next (rounded once) in
        the order quadratic, waypoint, pair-distance -- on the position features, the velocity features see the quadratic term only --
        and last, on the position features, g = g + ((tc * 2) * lap) / (L - 1) once with tc the sum of the terms' coefficients."""
        B, L, F = pos.shape
        nb = F // 4
        self.check_state(B, L, nb)
        g, have = torch.zeros_like(pos).reshape(B, L, nb, 4), False
        for t in self.table_terms(L, nb):
            gt = t._without_time_consistency().closed_form_grad(pos).reshape(B, L, nb, 4)
            if isinstance(t, QuadraticObjective):
                g = gt.clone()
            elif have:
                g[..., :2] = g[..., :2] + gt[..., :2]
            else:
                g[..., :2] = gt[..., :2]
            have = True
        if self.time_consistency_coef > 0 and L > 1:
            g[..., :2] = g[..., :2] + _TableObjective._time_consistency_grad(self, pos.reshape(B, L, nb, 4)[..., :2])
        return g.reshape(B, L, F)

    # ------------------------------------------------------------------ the library's guided chains
    def descriptor(self, design_guidance):
        """cindm_design_desc (mode 7; the tables are armed per call) under ``design_guidance``, or None when that guidance needs the
        generic (autograd) path.  In mode 7 ``last_n_step`` names the waypoint term's norm: 1 = L2, 2 = L2square, 0 without one."""
        parsed = _parse_guidance(design_guidance)
        if parsed is None:
            return None
        d = _ffi.DesignDesc()
        d.mode = 7
        d.alpha, d.recurrence = parsed
        way = [t for t in self.terms if _sum_kind(t) == "waypoint"]
        d.last_n_step = (1 if way[0].design_fn_mode == "L2" else 2) if way else 0
        d.time_consistency_coef = self.time_consistency_coef
        return d

    def arm(self, handle, B, device):
        """Arms the next guided chain call on ``handle`` with every term's tables, for the state ``check_state`` last saw."""
        terms = self.terms if self._last is None else self.table_terms(*self._last)
        if any(isinstance(t, PointObjective) for t in terms):
            raise RuntimeError("SumObjective.arm before check_state: a PointObjective term needs the state's (L, n_bodies)")
        for t in terms:
            t.arm(handle, B, device)
