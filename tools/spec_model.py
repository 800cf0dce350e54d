#!/usr/bin/env python3
"""m(k) of the speculative one-chunk pass, derived from a reference model instead of tuned on the library.

The model: the scores of one query against n uniformly random unit vectors in d dimensions (density ~ (1 - x^2)^((d - 3) / 2)).
The starter estimates their mean and standard deviation from a sample of S = 16 384 rows; the pass then screens all n rows at
    t = mu^ + sigma^ * zq,   zq = Phi^-1(1 - m / n)      (a GAUSSIAN quantile: the device never inverts a distribution)
and is exact when the k-th best score of the n rows is at or above t.  The miss margin of a query is
    (k-th best - t) / sigma^ = (k-th best - mu^) / sigma^ - zq.
Its mean and spread come from three independent sources, all worked out by quadrature (no sampling):
  * the k-th largest of n draws: its tail probability is Beta(k, n - k + 1), pushed through the exact quantile function;
  * mu^: variance sigma^2 / S;
  * sigma^: variance sigma^2 (kurtosis - 1) / (4 S), which moves the margin by (k-th best / sigma) times its relative error.
RULE: m(k) = the smallest m whose mean margin is at least kSigmas = 5 of its standard deviations at n = 2^20 AND at n = 10^7,
d = 768 (5: the headline tests assert retry_queries == 0 over a few thousand queries).  A pass may speculate at k only if
kInflation * m(k) <= 0.75 * (1024 - k): the one-wave prune's list, with the inflation the schedule budgets for the int8 bound.

`python tools/spec_model.py` prints the table; `--simulate` checks the quadrature against plain sampling of the same model.
Only NumPy and the standard library; nothing of the package is imported.
"""
from __future__ import annotations

import argparse
import math

import numpy as np

SAMPLE_ROWS = 16384
K_SIGMAS = 5.0
INFLATION = 10
PRUNE_ENTRIES = 1024
RULE_D = 768
RULE_NS = (1 << 20, 10_000_000)
K_TABLE_MAX = 32  # the starter serves k <= 32: no larger k can speculate


def norm_ppf(p: float) -> float:
    """Phi^-1(p) by bisection on erfc (the library's host code does the same)."""
    lo, hi = -40.0, 40.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if 0.5 * math.erfc(-mid / math.sqrt(2.0)) < p:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


class Scores:
    """One coordinate of a uniformly random unit vector in d dimensions: tail function, its inverse and the moments."""

    def __init__(self, d: int, grid: int = 400_001):
        self.d = d
        self.kth_cache: dict[tuple[int, int], tuple[float, float]] = {}
        x = np.linspace(0.0, 1.0, grid)
        with np.errstate(divide="ignore"):
            logf = 0.5 * (d - 3) * np.log1p(-x * x)
        f = np.exp(logf)
        f[-1] = 0.0
        seg = 0.5 * (f[1:] + f[:-1]) * (x[1] - x[0])
        tail = np.concatenate([np.cumsum(seg[::-1])[::-1], [0.0]])  # integral of f over [x, 1]
        total = 2.0 * tail[0]
        self.x = x
        self.tail = tail / total
        self.sigma = math.sqrt(1.0 / d)  # E x^2 = 1 / d exactly
        self.kurtosis = 3.0 * d / (d + 2.0)  # E x^4 = 3 / (d (d + 2))
        keep = self.tail > 1e-300
        self._logtail = np.log(self.tail[keep])[::-1]  # ascending for np.interp
        self._xs = x[keep][::-1]

    def quantile_of_tail(self, p: np.ndarray) -> np.ndarray:
        return np.interp(np.log(p), self._logtail, self._xs)

    def tail_at(self, xv: float) -> float:
        return float(np.interp(xv, self.x, self.tail))


def kth_best_moments(sc: Scores, n: int, k: int) -> tuple[float, float]:
    """mean and variance of the k-th largest of n draws: tail probability p ~ Beta(k, n - k + 1)"""
    if (n, k) not in sc.kth_cache:
        sc.kth_cache[n, k] = _kth_best_moments(sc, n, k)
    return sc.kth_cache[n, k]


def _kth_best_moments(sc: Scores, n: int, k: int) -> tuple[float, float]:
    mode = k / n
    p = np.exp(np.linspace(math.log(mode) - 12.0, math.log(mode) + 5.0, 20_001))
    p = p[p < 0.5]
    logw = (k - 1) * np.log(p) + (n - k) * np.log1p(-p) + np.log(p)  # density in log p
    w = np.exp(logw - logw.max())
    w /= w.sum()
    xk = sc.quantile_of_tail(p)
    mean = float((w * xk).sum())
    return mean, float((w * (xk - mean) ** 2).sum())


def margin(sc: Scores, n: int, k: int, m: float, sample: int = SAMPLE_ROWS) -> tuple[float, float, float]:
    """(mean, standard deviation) of the miss margin in units of sigma^, and the rows expected above t"""
    zq = norm_ppf(1.0 - m / n)
    mean_k, var_k = kth_best_moments(sc, n, k)
    zk = mean_k / sc.sigma
    var = var_k / sc.sigma**2 + 1.0 / sample + zk * zk * (sc.kurtosis - 1.0) / (4.0 * sample)
    return zk - zq, math.sqrt(var), n * sc.tail_at(zq * sc.sigma)


def budget_ok(k: int, m: int) -> bool:
    return m > 0 and INFLATION * m <= 0.75 * (PRUNE_ENTRIES - k)


def smallest_m(k: int, sc: Scores | None = None) -> int:
    """the rule, before the budget: the smallest m with mean margin >= 5 sd at both sizes (0: none below the list's size)"""
    sc = sc or Scores(RULE_D)
    for m in range(k + 1, PRUNE_ENTRIES):
        if all(mu >= K_SIGMAS * sd for mu, sd, _ in (margin(sc, n, k, m) for n in RULE_NS)):
            return m
    return 0


def table(kmax: int = K_TABLE_MAX) -> list[int]:
    """m(k) for k = 0 .. kmax as the library compiles it in: 0 where no admissible m exists"""
    sc = Scores(RULE_D)
    out = [0]
    for k in range(1, kmax + 1):
        m = smallest_m(k, sc)
        out.append(m if budget_ok(k, m) else 0)
    return out


def simulate(d: int, n: int, k: int, m: int, trials: int, seed: int = 1) -> tuple[float, float]:
    """the same model by sampling: S drawn scores for the moments, the k-th best of n through its Beta tail probability"""
    rng = np.random.default_rng(seed)
    sc = Scores(d)
    zq = norm_ppf(1.0 - m / n)
    out = np.empty(trials)
    for i in range(trials):
        g = rng.standard_normal(SAMPLE_ROWS)
        c = rng.chisquare(d - 1, SAMPLE_ROWS)
        xs = g / np.sqrt(g * g + c)
        p = rng.beta(k, n - k + 1)
        xk = float(sc.quantile_of_tail(np.array([p]))[0])
        out[i] = (xk - xs.mean()) / xs.std() - zq
    return float(out.mean()), float(out.std())


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--simulate", type=int, default=0, metavar="TRIALS", help="check k = 10 against sampling")
    args = ap.parse_args()
    sc = Scores(RULE_D)
    print(f"d = {RULE_D}, sample = {SAMPLE_ROWS} rows, rule: mean margin >= {K_SIGMAS:g} sd at n = {RULE_NS[0]} and {RULE_NS[1]}")
    print("  k    m  budget |" + "".join(f"  n={n:<9d} margin    sd  mean/sd  rows>t |" for n in RULE_NS))
    for k in range(1, K_TABLE_MAX + 1):
        m = smallest_m(k, sc)
        row = f"{k:3d} {m:4d}  {'ok ' if budget_ok(k, m) else 'no '}    |"
        for n in RULE_NS:
            mu, sd, above = margin(sc, n, k, m)
            row += f"              {mu:6.3f} {sd:6.3f} {mu / sd:7.2f} {above:7.1f} |"
        print(row)
    print("compiled-in table (k = 0 ..):", table())
    if args.simulate:
        for n in RULE_NS:
            for m in (42, 60, 80):
                mu, sd, _ = margin(sc, n, 10, m)
                smu, ssd = simulate(RULE_D, n, 10, m, args.simulate)
                print(f"k = 10, m = {m}, n = {n}: quadrature {mu:.3f} / {sd:.3f} = {mu / sd:.2f}; sampled {smu:.3f} / {ssd:.3f} = {smu / ssd:.2f}")


if __name__ == "__main__":
    main()
