"""Host-only fp64 restatement of the RMSprop op of k_optim_step (csrc/meshenv_optim.h: kOptRmsprop): one step of
``torch.optim.rmsprop._single_tensor_rmsprop`` with momentum = 0 and centered = False, with a per-element bound on the float32
error, a float32 restatement and named mistakes.  Shared by tests/test_rmsprop_cpu.py, tests/test_gpu_policy_step.py and
tools/bench_ppo_epoch.py; nothing here touches a device.

The statement.  From float32 ``(p, v, g)`` (v is ``square_avg``) and the scalars of ``scalars(lr, alpha, eps)`` -- Python
doubles rounded to float32, which is what the host passes to the kernel and what torch's kernels receive; the fp64
restatement uses those same float-rounded values, so that rounding is not part of the error --

    a   = v al;  b = (w2 g) g                    mul; mul, mul               al = fl(alpha), w2 = fl(1 - alpha)
    v'  = a + b                                  add
    s   = sqrt(v')                               sqrt (correctly rounded)
    den = s + eps                                add
    r   = g / den                                div (correctly rounded)
    p'  = p + (-lr) r                            mul, add                    lr = fl(lr)

The bound is built from the rules of tests/optim_step_ref.py (``_mul``, ``_add``, ``_sqrt``, ``_div``; u = 2^-24, eta = 2^-149),
imported, not restated: they are the same float32 operations, and its remark on contraction holds here as it does there (the
kernel contracts nothing; torch's kernels may).  ``den >= eps (1 - u) > 0`` whatever v' is, so ``_div`` applies; at v' = 0
exactly (g = 0 and v = 0) every term of the root's bound is 0, s = 0 is exact, r = 0 and the restated p' is p.

Non-finite gradients are outside the analysis: the tests compare the SET of non-finite outputs with stock torch's and apply the
bound to the other elements."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from optim_step_ref import SHAPES, _add, _c, _div, _mul, _sqrt, assert_within, f32, flat_grads, ratio, tensors, worst  # noqa: F401
from policy_ref import _f64

LR, ALPHA, EPS = 7e-4, 0.99, 1e-5                              # SB3's A2C: RMSprop(alpha=0.99, eps=1e-5), learning_rate 7e-4
MUTANTS = ("eps_inside_sqrt", "alpha_swapped", "v_from_g", "sign_of_update", "adam_bias_correction")
KEYS = ("p", "square_avg")

Scalars = namedtuple("Scalars", "lr al w2 eps")               # float32 values held as Python floats


def scalars(lr=LR, alpha=ALPHA, eps=EPS, mutant=None) -> Scalars:
    """The float32 scalars of a step: lr, alpha, 1 - alpha (formed in doubles, as torch forms ``value=1 - alpha``), eps."""
    al, w2 = alpha, 1 - alpha
    if mutant == "alpha_swapped":
        al, w2 = w2, al
    return Scalars(f32(lr), f32(al), f32(w2), f32(eps))


def rmsprop(p, v, g, sc: Scalars, mutant=None, step=1):
    """{"p", "square_avg"} -> (ref, bound) after one step from (p, v, g) with the scalars sc.  ``step``: what the
    adam_bias_correction mistake divides by (1 - alpha^step)."""
    P, V, G = ((_f64(x), 0.0) for x in (p, v, g))
    ok = mutant is None                   # a mistake may divide by anything: only its value is used
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        second = _mul(_c(sc.w2), G) if mutant == "v_from_g" else _mul(_mul(_c(sc.w2), G), G)
        v1 = _add(_mul(V, _c(sc.al)), second)
        root = v1
        if mutant == "adam_bias_correction":           # Adam's denominator: sqrt(v / (1 - alpha^step))
            root = _div(v1, _c(f32(1 - sc.al ** step)), ok)
        if mutant == "eps_inside_sqrt":                # RMSpropTFLike's order
            den = _sqrt(_add(root, _c(sc.eps)))
        else:
            den = _add(_sqrt(root), _c(sc.eps))
        r = _div(G, den, ok)
        p1 = _add(P, _mul(_c(sc.lr if mutant == "sign_of_update" else -sc.lr), r))
    return {"p": p1, "square_avg": v1}


def rmsprop_f32(p, v, g, sc: Scalars):
    """The same sequence in numpy float32, one rounding per operation, nothing contracted."""
    f = np.float32
    p, v, g = (np.asarray(x, f) for x in (p, v, g))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        v1 = v * f(sc.al) + (f(sc.w2) * g) * g
        den = np.sqrt(v1) + f(sc.eps)
        p1 = p + f(-sc.lr) * (g / den)
    return {"p": p1, "square_avg": v1}


def state(shape, seed, loaded=False):
    """float32 (p, v, g) of one tensor: optim_step_ref.tensors' parameters, second moments and gradients (exact zeros at every
    seventh element, v = 0 there when ``loaded``); else the empty state v = 0."""
    p, _, v, g = tensors(shape, seed, loaded=loaded)
    return p, v, g
