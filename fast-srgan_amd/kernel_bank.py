"""The blur kernels of the high-order degradation model, built on the host in float64 numpy: the taps ops.filter2d
(csrc/degrade.hip: filter2d_kernel) applies per sample.  No scipy: J1 is evaluated here.

With u = (j - c, i - c) the offset of tap [i][j] from the centre c = (K - 1) / 2 (x along a row, y down a column),
S = R(theta) diag(sx^2, sy^2) R(theta)^T and q = u^T S^-1 u:
    gauss        exp(-q / 2)
    generalized  exp(-q^beta / 2)
    plateau      1 / (1 + q^beta)
each as "iso" (sx = sy, theta = 0) or "aniso", and
    sinc         omega J1(omega |u|) / (2 pi |u|), omega^2 / (4 pi) at the centre     (the ideal circular low-pass of cut-off omega: ringing)
Every kernel is divided by its sum in float64 and cast to float32.
"""
import math

import numpy as np

KINDS = ("iso", "aniso", "generalized_iso", "generalized_aniso", "plateau_iso", "plateau_aniso")
MAX_SIZE = 21


def j1(x):
    """The Bessel function J1 by Bessel's integral, J1(x) = (1 / 2 pi) int_-pi^pi cos(t - x sin t) dt, with the trapezoid rule on 128
    points of the period: the integrand is periodic and entire, so the rule's error is the aliasing sum of J_m(x), |m| >= 127, far
    below 1e-16 on [0, 10 pi] (the argument range of a 21 x 21 sinc kernel at omega = pi is 10 sqrt(2) pi; checked to 50)."""
    x = np.asarray(x, dtype=np.float64)
    t = (2.0 * math.pi / 128.0) * np.arange(128, dtype=np.float64)
    return np.cos(t - x[..., None] * np.sin(t)).mean(axis=-1)


def _offsets(size):
    if size % 2 != 1 or not 1 <= size <= MAX_SIZE:
        raise ValueError("kernel size must be odd and lie in 1..%d, got %r" % (MAX_SIZE, size))
    c = (size - 1) / 2.0
    i, j = np.mgrid[0:size, 0:size].astype(np.float64)
    return j - c, i - c                                             # x, y


def _q(size, sigma_x, sigma_y, theta):
    if not (sigma_x > 0 and sigma_y > 0):
        raise ValueError("kernel sigmas must be positive, got %r, %r" % (sigma_x, sigma_y))
    x, y = _offsets(size)
    co, si = math.cos(theta), math.sin(theta)
    a, b = co * x + si * y, -si * x + co * y                         # R^T u
    return (a / sigma_x) ** 2 + (b / sigma_y) ** 2


def _normalised(k, dtype):
    return (k / k.sum()).astype(dtype)


def bank_kernel(kind, size, sigma_x, sigma_y=None, theta=0.0, beta=1.0, dtype=np.float32):
    """One kernel of the bank as a float32 (size, size) array.  kind: one of KINDS; an "iso" kind ignores sigma_y and theta, a plain
    Gaussian ignores beta.  dtype=np.float64 returns the normalised kernel before the cast (what the tests hold to the formulas)."""
    if kind not in KINDS:
        raise ValueError("kernel kind must be one of %s, got %r" % (", ".join(KINDS), kind))
    if kind.endswith("iso") and not kind.endswith("aniso"):
        sigma_y, theta = sigma_x, 0.0
    elif sigma_y is None:
        sigma_y = sigma_x
    q = _q(int(size), float(sigma_x), float(sigma_y), float(theta))
    if kind.startswith("generalized"):
        k = np.exp(-0.5 * q ** float(beta))
    elif kind.startswith("plateau"):
        k = 1.0 / (1.0 + q ** float(beta))
    else:
        k = np.exp(-0.5 * q)
    return _normalised(k, dtype)


def sinc_kernel(omega, size, dtype=np.float32):
    """The circular low-pass filter of cut-off omega (0 < omega <= pi) as a float32 (size, size) array (dtype: as in bank_kernel)."""
    if not 0.0 < omega <= math.pi + 1e-12:
        raise ValueError("sinc cut-off must lie in (0, pi], got %r" % (omega,))
    x, y = _offsets(int(size))
    rad = np.sqrt(x * x + y * y)
    safe = np.where(rad > 0, rad, 1.0)
    k = np.where(rad > 0, omega * j1(omega * safe) / (2.0 * math.pi * safe), omega * omega / (4.0 * math.pi))
    return _normalised(k, dtype)


def _pair(v, what, lo=None):
    v = tuple(float(x) for x in v)
    if len(v) != 2 or not v[0] <= v[1] or (lo is not None and not v[0] > lo):
        raise ValueError("%s must be a (lo, hi) pair with %slo <= hi, got %r" % (what, "" if lo is None else "%g < " % lo, v))
    return v


class KernelBank:
    """The distribution a stage's blur kernels are drawn from.  kernel_size: (lo, hi), the odd sizes in it are equally likely;
    kernel_kinds: one weight per entry of KINDS; kernel_sigma in pixels of the resolution the stage runs at; kernel_beta_generalized /
    kernel_beta_plateau: the shape ranges; sinc_prob: how often a sinc kernel replaces the bank's choice (omega uniform in [pi/3, pi] below
    size 13, else [pi/5, pi])."""

    def __init__(self, kernel_size=(7, 21), kernel_kinds=(0.45, 0.25, 0.12, 0.03, 0.12, 0.03), kernel_sigma=(0.2, 3.0),
                 kernel_beta_generalized=(0.5, 4.0), kernel_beta_plateau=(1.0, 2.0), sinc_prob=0.0):
        lo, hi = (int(v) for v in kernel_size)
        self.sizes = [k for k in range(lo, hi + 1) if k % 2 == 1]
        if len(tuple(kernel_size)) != 2 or not self.sizes or self.sizes[0] < 1 or self.sizes[-1] > MAX_SIZE:
            raise ValueError("kernel_size must be a (lo, hi) pair holding an odd size in 1..%d, got %r" % (MAX_SIZE, kernel_size))
        self.kernel_size = (lo, hi)
        self.kernel_kinds = tuple(float(v) for v in kernel_kinds)
        if len(self.kernel_kinds) != len(KINDS) or min(self.kernel_kinds) < 0 or not sum(self.kernel_kinds) > 0:
            raise ValueError("kernel_kinds must hold %d non-negative weights (%s), not all 0, got %r" % (len(KINDS), ", ".join(KINDS), kernel_kinds))
        self.kernel_sigma = _pair(kernel_sigma, "kernel_sigma", 0.0)
        self.kernel_beta_generalized = _pair(kernel_beta_generalized, "kernel_beta_generalized", 0.0)
        self.kernel_beta_plateau = _pair(kernel_beta_plateau, "kernel_beta_plateau", 0.0)
        self.sinc_prob = float(sinc_prob)
        if not 0.0 <= self.sinc_prob <= 1.0:
            raise ValueError("sinc_prob must be a probability, got %r" % (sinc_prob,))

    def draw(self, rng):
        """The parameters of one kernel from `rng` (a random.Random): always the same nine variates in the same order -- size, kind,
        sigma_x, sigma_y, theta, the two betas, the sinc decision, omega's variate -- whatever kind comes out."""
        size = self.sizes[int(rng.random() * len(self.sizes))]       # (randrange would consume a varying number of words)
        u, kind, acc = rng.random() * sum(self.kernel_kinds), KINDS[-1], 0.0
        for name, wt in zip(KINDS, self.kernel_kinds):
            acc += wt
            if u < acc:
                kind = name
                break
        sx, sy = rng.uniform(*self.kernel_sigma), rng.uniform(*self.kernel_sigma)
        theta = rng.uniform(-math.pi, math.pi)
        bg, bp = rng.uniform(*self.kernel_beta_generalized), rng.uniform(*self.kernel_beta_plateau)
        sinc, v = rng.random() < self.sinc_prob, rng.random()
        if sinc:
            lo = math.pi / 3.0 if size < 13 else math.pi / 5.0
            return {"kind": "sinc", "size": size, "omega": lo + v * (math.pi - lo)}
        beta = bg if kind.startswith("generalized") else (bp if kind.startswith("plateau") else 1.0)
        return {"kind": kind, "size": size, "sigma_x": sx, "sigma_y": sy, "theta": theta, "beta": beta}


def draw_sinc(rng, size):
    """The parameters of a final sinc filter of the given size: omega by draw()'s rule."""
    lo = math.pi / 3.0 if size < 13 else math.pi / 5.0
    return {"kind": "sinc", "size": size, "omega": lo + rng.random() * (math.pi - lo)}


def build(params):
    """The float32 kernel of the parameters draw() returned; None stays None (the stage did not fire: the sample is copied)."""
    if params is None:
        return None
    if params["kind"] == "sinc":
        return sinc_kernel(params["omega"], params["size"])
    return bank_kernel(params["kind"], params["size"], params["sigma_x"], params["sigma_y"], params["theta"], params["beta"])
