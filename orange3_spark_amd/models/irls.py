"""Generalized linear models by iteratively reweighted least squares (Spark's
GeneralizedLinearRegression, solver "irls").

Each IRLS iteration is one pass over the rank's rows: the working response and weights
are elementwise, the weighted normal equations ``[X 1]^T W [X 1]`` / ``[X 1]^T W z`` are
one chunked GEMM each (hipBLASLt on the GPU), and the (D+1)^2 + (D+1) + 2 statistics are
summed across ranks with ONE all-reduce; the small SPD solve runs in fp64 on the host.
Families: gaussian, binomial, poisson, gamma, tweedie; links: identity, log, logit,
probit, cloglog, inverse, sqrt and the tweedie power link.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from ..ops.gram import rows_t_matmul, weighted_gram
from ..runtime import progress

_DEFAULT_LINK = {"gaussian": "identity", "binomial": "logit", "poisson": "log", "gamma": "inverse"}
_EPS = 1e-16


class Link:
    def __init__(self, name: str, power: float | None = None):
        self.name, self.power = name, power

    def link(self, mu):
        n = self.name
        if n == "identity":
            return mu
        if n == "log":
            return torch.log(mu)
        if n == "logit":
            return torch.log(mu / (1 - mu))
        if n == "probit":
            return math.sqrt(2.0) * torch.special.erfinv(2 * mu - 1)
        if n == "cloglog":
            return torch.log(-torch.log1p(-mu))
        if n == "inverse":
            return 1.0 / mu
        if n == "sqrt":
            return torch.sqrt(mu)
        if n == "power":
            return torch.log(mu) if self.power == 0 else mu ** self.power
        raise ValueError(f"unknown link {n}")

    def unlink(self, eta):
        n = self.name
        if n == "identity":
            return eta
        if n == "log":
            return torch.exp(eta)
        if n == "logit":
            return torch.sigmoid(eta)
        if n == "probit":
            return 0.5 * (1 + torch.erf(eta / math.sqrt(2.0)))
        if n == "cloglog":
            return 1 - torch.exp(-torch.exp(eta))
        if n == "inverse":
            return 1.0 / eta
        if n == "sqrt":
            return eta * eta
        if n == "power":
            return torch.exp(eta) if self.power == 0 else eta ** (1.0 / self.power)
        raise ValueError(f"unknown link {n}")

    def deriv(self, mu):
        """d eta / d mu."""
        n = self.name
        if n == "identity":
            return torch.ones_like(mu)
        if n == "log":
            return 1.0 / mu
        if n == "logit":
            return 1.0 / (mu * (1 - mu))
        if n == "probit":
            eta = self.link(mu)
            return math.sqrt(2 * math.pi) * torch.exp(0.5 * eta * eta)
        if n == "cloglog":
            return 1.0 / ((mu - 1) * torch.log1p(-mu))
        if n == "inverse":
            return -1.0 / (mu * mu)
        if n == "sqrt":
            return 0.5 / torch.sqrt(mu)
        if n == "power":
            return 1.0 / mu if self.power == 0 else self.power * mu ** (self.power - 1)
        raise ValueError(f"unknown link {n}")


class Family:
    def __init__(self, name: str, variance_power: float = 0.0):
        self.name, self.p = name, variance_power

    def variance(self, mu):
        n = self.name
        if n == "gaussian":
            return torch.ones_like(mu)
        if n == "binomial":
            return mu * (1 - mu)
        if n == "poisson":
            return mu
        if n == "gamma":
            return mu * mu
        return mu ** self.p

    def initialize(self, y, w):
        n = self.name
        if n == "binomial":
            return (w * y + 0.5) / (w + 1.0)
        if n == "poisson":
            return torch.clamp(y, min=0.1)
        if n in ("gamma",):
            return torch.clamp(y, min=_EPS)
        if n == "tweedie":
            return torch.where(y == 0, torch.full_like(y, 0.1), y) if self.p >= 1 else y
        return y

    def clean(self, mu):
        if self.name == "binomial":
            return mu.clamp(_EPS, 1 - _EPS)
        if self.name in ("poisson", "gamma") or (self.name == "tweedie" and self.p >= 1):
            return mu.clamp_min(_EPS)
        return mu

    def deviance(self, y, mu, w):
        n = self.name
        if n == "gaussian":
            return w * (y - mu) ** 2
        if n == "binomial":
            def ylogy(a, b):
                return torch.where(a > 0, a * torch.log(a / b), torch.zeros_like(a))
            return 2 * w * (ylogy(y, mu) + ylogy(1 - y, 1 - mu))
        if n == "poisson":
            t = torch.where(y > 0, y * torch.log(y / mu), torch.zeros_like(y))
            return 2 * w * (t - (y - mu))
        if n == "gamma":
            return -2 * w * (torch.log(torch.clamp(y, min=_EPS) / mu) - (y - mu) / mu)
        p = self.p
        if p == 0:
            return w * (y - mu) ** 2
        if p == 1:
            return Family("poisson").deviance(y, mu, w)
        if p == 2:
            return Family("gamma").deviance(y, mu, w)
        y1 = torch.clamp(y, min=0) if p < 2 else torch.clamp(y, min=_EPS)
        return 2 * w * (y1 ** (2 - p) / ((1 - p) * (2 - p)) - y * mu ** (1 - p) / (1 - p)
                        + mu ** (2 - p) / (2 - p))


def make_link(family: str, link: str | None, variance_power: float, link_power: float | None) -> Link:
    if family == "tweedie":
        lp = (1.0 - variance_power) if link_power is None else link_power
        if lp == 1.0:
            return Link("identity")
        if lp == 0.0:
            return Link("log")
        if lp == -1.0:
            return Link("inverse")
        if lp == 0.5:
            return Link("sqrt")
        return Link("power", lp)
    return Link(link or _DEFAULT_LINK[family])


@dataclass
class IrlsResult:
    coef: np.ndarray
    intercept: float
    iterations: int
    deviance: float
    null_deviance: float
    dispersion: float
    cov_unscaled: np.ndarray | None
    rank: int
    n_obs: float
    log_likelihood_terms: float


def fit_irls(comm, X: torch.Tensor, y: torch.Tensor, w: torch.Tensor | None, offset: torch.Tensor | None,
             family: Family, link: Link, fit_intercept=True, reg=0.0, max_iter=25, tol=1e-6,
             chunk=1 << 20, rows: torch.Tensor | None = None) -> IrlsResult:
    """``rows``: the stored rows of the feature column (X is their ``[:, :D]`` view) when the fused
    Gram pass takes them (ops.gram.column_rows): each iteration's normal equations are then one
    ``weighted_gram`` over them instead of fp64 chunk copies."""
    dev = X.device
    dt = torch.float64
    n, D = X.shape
    y = y.to(dev, dt)
    w = torch.ones(n, dtype=dt, device=dev) if w is None else w.to(dev, dt)
    off = torch.zeros(n, dtype=dt, device=dev) if offset is None else offset.to(dev, dt)
    P = D + (1 if fit_intercept else 0)

    def normal_eq(z, ww):
        A = torch.zeros((P, P), dtype=dt, device=dev)
        bvec = torch.zeros(P, dtype=dt, device=dev)
        if rows is not None:
            gs = weighted_gram(rows, D, w=ww, y=z)
            A[:D, :D], bvec[:D] = gs.G, gs.xty
            if fit_intercept:
                A[:D, D] = A[D, :D] = gs.sx
                A[D, D], bvec[D] = gs.sw, gs.sy
            buf = torch.cat([A.reshape(-1), bvec, gs.sw[None]])
            comm.all_reduce(buf)
            return buf[: P * P].reshape(P, P).cpu().numpy(), buf[P * P: P * P + P].cpu().numpy(), float(buf[-1])
        for a in range(0, n, chunk):
            b = min(n, a + chunk)
            Xc = X[a:b].to(dt)
            if fit_intercept:
                Xc = torch.cat([Xc, torch.ones((b - a, 1), dtype=dt, device=dev)], dim=1)
            wc = ww[a:b]
            A += rows_t_matmul(Xc * wc[:, None], Xc)        # block-batched: not a 1-tile GEMM
            bvec += rows_t_matmul(Xc, wc * z[a:b])
        buf = torch.cat([A.reshape(-1), bvec, ww.sum()[None]])
        comm.all_reduce(buf)
        return buf[: P * P].reshape(P, P).cpu().numpy(), buf[P * P: P * P + P].cpu().numpy(), float(buf[-1])

    def eta_of(beta):
        e = off.clone()
        for a in range(0, n, chunk):
            b = min(n, a + chunk)
            e[a:b] += X[a:b].to(dt) @ torch.from_numpy(beta[:D]).to(dev, dt)
        if fit_intercept:
            e += float(beta[D])
        return e

    mu = family.clean(family.initialize(y, w))
    eta = link.link(mu)
    beta = np.zeros(P)
    it = 0
    cov = None
    for it in range(1, max_iter + 1):
        progress.iteration(it - 1, max_iter)
        dmu = 1.0 / link.deriv(mu)                      # d mu / d eta
        z = eta - off + (y - mu) / dmu
        ww = w * dmu * dmu / family.variance(mu)
        A, bv, sw = normal_eq(z, ww)
        if reg > 0:
            A[:D, :D] += reg * sw * np.eye(D)
        try:
            new = np.linalg.solve(A, bv)
            cov = np.linalg.inv(A)
        except np.linalg.LinAlgError:
            new = np.linalg.lstsq(A, bv, rcond=None)[0]
            cov = np.linalg.pinv(A)
        delta = np.max(np.abs(new - beta)) / max(np.max(np.abs(beta)), 1e-12) if it > 1 else np.inf
        beta = new
        eta = eta_of(beta)
        mu = family.clean(link.unlink(eta))
        if delta < tol:
            break
    dev_sum = family.deviance(y, mu, w).sum()
    # null model: intercept only (weighted mean through the link), or mu = link^-1(offset)
    if fit_intercept:
        s = torch.stack([(w * y).sum(), w.sum()])
        comm.all_reduce(s)
        ybar = float(s[0] / s[1])
        mu0 = family.clean(torch.full_like(y, ybar)) if offset is None else family.clean(
            link.unlink(off + link.link(torch.tensor(ybar, dtype=dt, device=dev))))
    else:
        mu0 = family.clean(link.unlink(off))
    stats = torch.stack([dev_sum, family.deviance(y, mu0, w).sum(), w.sum(), torch.tensor(float(n), device=dev,
                                                                                       dtype=dt)])
    # Pearson chi^2 for the dispersion estimate
    pear = (w * (y - mu) ** 2 / family.variance(mu)).sum()
    stats = torch.cat([stats, pear[None]])
    comm.all_reduce(stats)
    dev_sum, null_dev, wsum, nobs, pear = (float(v) for v in stats)
    df_resid = nobs - P
    if family.name in ("binomial", "poisson"):
        disp = 1.0
    else:
        disp = pear / max(df_resid, 1.0)
    coef = beta[:D]
    b0 = float(beta[D]) if fit_intercept else 0.0
    return IrlsResult(coef, b0, it, dev_sum, null_dev, disp, cov, P, nobs, wsum)
