"""Host-only fp64 restatement of k_optim_step (csrc/meshenv_optim.h): one Adam step and one Polyak update, each with a
per-element bound on the float32 error, a float32 restatement, and named mistakes.  Shared by tests/test_optim_step_cpu.py,
tests/test_gpu_optim_step.py and tools/bench_optim_step.py; nothing here touches a device.

The statement.  From float32 ``(p, m, v, g)`` and the scalars of ``scalars(step, lr, beta1, beta2, eps)`` -- computed in
Python doubles from the INCREMENTED step exactly as ``torch.optim.adam._single_tensor_adam`` does and then rounded to float32,
which is what the host passes to the kernel; the fp64 restatement uses those same float-rounded values, so that rounding is
not part of the error --

    d   = g - m                                  add
    m'  = m + d w1                               mul, add                    w1 = fl(1 - beta1)
    a   = v b2;  b = (w2 g) g                    mul; mul, mul               b2 = fl(beta2), w2 = fl(1 - beta2)
    v'  = a + b                                  add
    s   = sqrt(v')                               sqrt (correctly rounded)
    q   = s / c2                                 div (correctly rounded)     c2 = fl((1 - beta2^step)^0.5)
    den = q + eps                                add
    r   = m' / den                               div
    p'  = p + (-ss) r                            mul, add                    ss = fl(lr / (1 - beta1^step))
    t'  = t omt + tau p                          mul, mul, add               omt = fl(1 - tau), tau = fl(tau)

The bound, by forward error analysis (u = 2^-24, eta = 2^-149).  Every quantity is a pair (x, e): the fp64 value and a bound
on |float32 value - x|.  The inputs and the scalars are exact (e = 0).  One float32 operation adds u times the largest
magnitude its exact result can have, given its operands' bounds, to the propagated error; a product also adds eta, the most
gradual underflow can cost (sums of float32 numbers are exact in the subnormal range):

    mul   (a, ea)(b, eb):  |a| eb + |b| ea + ea eb + u (|a| + ea)(|b| + eb) + eta
    add   (a, ea) + (b, eb):  ea + eb + u (|a + b| + ea + eb)
    sqrt  (a, ea), a >= 0:  s - sqrt(max(a - ea, 0)) + u sqrt(a + ea)              the concave side is the larger one
    div   (a, ea) / (b, eb), lo = |b| - eb > 0:  ea / lo + |a| eb / (|b| lo) + u (|a| + ea) / lo + eta

A multiply-add pair may be contracted into one fma: the fma rounds once, and its error, the propagated part plus u times the
magnitude of the sum, is no larger than what the two bounds above add up to (the product's own u |a b| and eta terms are
simply not incurred).  So the bound holds for every choice of contraction in m', v', p' and t' (the kernel contracts none:
-ffp-contract=off; torch's kernels may).  The error of m' and v' is carried into p' through r and den: den >= eps (1 - u) > 0
whatever v' is, so ``div`` applies.  At v' = 0 exactly (g = 0 and v = 0) every term of its bound is 0 and s = 0 is exact.

Non-finite gradients are outside the analysis: the tests compare the SET of non-finite outputs with stock torch's and apply
the bound to the other elements.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from policy_ref import U, _f64, assert_within, ratio  # noqa: F401  (re-exported for the tests)

ETA = 2.0 ** -149
SHAPES = ((1,), (3,), (63,), (64,), (65,), (4097,), (128, 21))      # the tensors of the shape tests
LR, BETAS, EPS = 3e-4, (0.9, 0.999), 1e-8                          # SB3's Adam
ADAM_MUTANTS = ("drop_bias_correction1", "bias_correction2_not_rooted", "eps_inside_sqrt", "betas_swapped", "stale_step",
                "v_from_g", "sign_of_update")
POLYAK_MUTANTS = ("tau_swapped",)
FUSED_MUTANTS = ("polyak_before_adam",)
MUTANTS = ADAM_MUTANTS + POLYAK_MUTANTS + FUSED_MUTANTS

Scalars = namedtuple("Scalars", "ss c2 w1 b2 w2 eps")       # float32 values held as Python floats


def f32(x) -> float:
    with np.errstate(over="ignore"):
        return float(np.float32(x))


# ----------------------------------------------------------------------------------------------------------- host scalars
def torch_doubles(step, lr=LR, beta1=BETAS[0], beta2=BETAS[1]):
    """(step_size, bias_correction2_sqrt) in doubles: the four lines of _single_tensor_adam, transcribed."""
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    with np.errstate(divide="ignore"):
        step_size = float(np.float64(lr) / np.float64(bias_correction1))      # inf at step 0 (the stale_step mutant), no raise
    bias_correction2_sqrt = bias_correction2 ** 0.5
    return step_size, bias_correction2_sqrt


def scalars(step, lr=LR, beta1=BETAS[0], beta2=BETAS[1], eps=EPS, mutant=None) -> Scalars:
    """The float32 scalars the host passes for the step that ends at ``step`` (the incremented value)."""
    if mutant == "betas_swapped":
        beta1, beta2 = beta2, beta1
    ss, c2 = torch_doubles(step - 1 if mutant == "stale_step" else step, lr, beta1, beta2)
    if mutant == "drop_bias_correction1":
        ss = lr
    if mutant == "bias_correction2_not_rooted":
        c2 = c2 * c2
    return Scalars(f32(ss), f32(c2), f32(1 - beta1), f32(beta2), f32(1 - beta2), f32(eps))


# ----------------------------------------------------------------------------------------------------------- fp32 operations
def _c(x):
    return (np.float64(x), 0.0)


def _mul(x, y):
    (a, ea), (b, eb) = x, y
    return a * b, np.abs(a) * eb + np.abs(b) * ea + ea * eb + U * (np.abs(a) + ea) * (np.abs(b) + eb) + ETA


def _add(x, y):
    (a, ea), (b, eb) = x, y
    return a + b, ea + eb + U * (np.abs(a + b) + ea + eb)


def _sqrt(x):
    a, ea = x
    s = np.sqrt(a)
    lo = np.sqrt(np.maximum(a - ea, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        below = np.where(s + lo > 0, (a - np.maximum(a - ea, 0.0)) / (s + lo), 0.0)      # s - lo without the cancellation
    return s, below + U * np.sqrt(a + ea)


def _div(x, y, check=True):
    (a, ea), (b, eb) = x, y
    lo = np.abs(b) - eb
    assert not check or np.all(lo > 0), "division by an interval that contains 0"
    return a / b, ea / lo + np.abs(a) * eb / (np.abs(b) * lo) + U * (np.abs(a) + ea) / lo + ETA


# ----------------------------------------------------------------------------------------------------------- the restatement
def adam(p, m, v, g, sc: Scalars, mutant=None):
    """{"p", "exp_avg", "exp_avg_sq"} -> (ref, bound) after one step from (p, m, v, g) with the scalars sc."""
    P, M, V, G = ((_f64(x), 0.0) for x in (p, m, v, g))
    ok = mutant is None                   # a mistake may divide by anything: only its value is used
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m1 = _add(M, _mul(_add(G, (-M[0], 0.0)), _c(sc.w1)))
        second = _mul(_c(sc.w2), G) if mutant == "v_from_g" else _mul(_mul(_c(sc.w2), G), G)
        v1 = _add(_mul(V, _c(sc.b2)), second)
        if mutant == "eps_inside_sqrt":
            den = _div(_sqrt(_add(v1, _c(sc.eps))), _c(sc.c2), ok)
        else:
            den = _add(_div(_sqrt(v1), _c(sc.c2), ok), _c(sc.eps))
        r = _div(m1, den, ok)
        p1 = _add(P, _mul(_c(sc.ss if mutant == "sign_of_update" else -sc.ss), r))
    return {"p": p1, "exp_avg": m1, "exp_avg_sq": v1}


def polyak(t, p, tau, mutant=None):
    """(ref, bound) of t' = t (1 - tau) + tau p with the float32 scalars fl(1 - tau) and fl(tau)."""
    omt, ta = f32(1 - tau), f32(tau)
    if mutant == "tau_swapped":
        omt, ta = ta, omt
    return _add(_mul((_f64(t), 0.0), _c(omt)), _mul(_c(ta), (_f64(p), 0.0)))


def fused(p, m, v, g, t, sc: Scalars, tau, p_after=None, mutant=None):
    """Adam followed by Polyak of the same element.  The target reads the float32 parameter the step STORED: ``p_after``
    (the evaluation's own p') where given, so that the Polyak bound does not have to carry the step's; else fl(p' ref)."""
    out = adam(p, m, v, g, sc)
    if mutant == "polyak_before_adam":
        src = np.asarray(p, np.float32)
    else:
        src = np.asarray(p_after, np.float32) if p_after is not None else out["p"][0].astype(np.float32)
    out["target"] = polyak(t, src, tau)
    return out


# ----------------------------------------------------------------------------------------------------------- fp32 restatement
def adam_f32(p, m, v, g, sc: Scalars):
    """The same sequence in numpy float32, one rounding per operation, nothing contracted."""
    f = np.float32
    p, m, v, g = (np.asarray(x, f) for x in (p, m, v, g))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m1 = m + (g - m) * f(sc.w1)
        v1 = v * f(sc.b2) + (f(sc.w2) * g) * g
        den = np.sqrt(v1) / f(sc.c2) + f(sc.eps)
        p1 = p + f(-sc.ss) * (m1 / den)
    return {"p": p1, "exp_avg": m1, "exp_avg_sq": v1}


def polyak_f32(t, p, tau):
    f = np.float32
    return np.asarray(t, f) * f(1 - tau) + f(tau) * np.asarray(p, f)


# ----------------------------------------------------------------------------------------------------------- inputs
def tensors(shape, seed, loaded=False):
    """float32 (p, m, v, g) of one tensor: parameters of order 0.1, gradients of order 1e-2 with exact zeros at every
    seventh element; ``loaded``: moments such as six steps leave (m of order 5e-3, v of order 5e-7), and v = 0 with m = 0 or
    m = 1e-10 where the gradient is 0; else the empty state m = v = 0."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    p = (0.1 * rng.standard_normal(n)).astype(np.float32)
    g = (1e-2 * rng.standard_normal(n)).astype(np.float32)
    zero = np.arange(n) % 7 == 3 if n > 3 else np.arange(n) == n - 1 if n == 3 else np.zeros(n, bool)
    g[zero] = 0.0
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    if loaded:
        m = (5e-3 * rng.standard_normal(n)).astype(np.float32)
        v = (5e-7 * rng.uniform(0.2, 1.0, n)).astype(np.float32)
        v[zero] = 0.0
        m[zero] = np.where(np.arange(n)[zero] % 2 == 0, 0.0, 1e-10).astype(np.float32)
    return tuple(x.reshape(shape) for x in (p, m, v, g))


def targets(shape, seed):
    return (0.1 * np.random.default_rng(seed + 1000).standard_normal(int(np.prod(shape)))).astype(np.float32).reshape(shape)


def flat_grads(torch, params, device, lead=1):
    """Give every parameter a .grad that is a view into ONE flat buffer, the tensors back to back after ``lead`` floats: as
    FusedActorGrad hands them out, some of them off 16-byte alignment.  Returns the buffer."""
    total = lead + sum(p.numel() for p in params)
    buf = torch.zeros(total, dtype=torch.float32, device=device)
    at = lead
    for p in params:
        p.grad = buf[at:at + p.numel()].view(p.shape)
        at += p.numel()
    return buf


def worst(got, ref, what, out=None):
    """assert every entry of ref present in got within its bound; returns / records the largest ratio."""
    top = 0.0
    for k, rb in ref.items():
        if k in got:
            x = got[k]
            x = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
            r = assert_within(x.reshape(rb[0].shape), rb, f"{what} {k}")
            top = max(top, r)
            if out is not None:
                out[k] = max(out.get(k, 0.0), r)
    return top
