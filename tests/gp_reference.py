"""NumPy float64 restatement of the reference's RBF GP (train.py:60-150, GP_train_and_test): the oracle of the gp tests.

Written from the model's definition, not from the reference's code:
  (amp, noise, ls) = softplus(raw),  K_ij = exp(-|x_i / ls - x_j / ls|^2),  A = amp K + (noise + 1e-6) I,  y <- y - mean(y)
  NLML = 1/2 y^T A^-1 y + sum log L_ii + (N/2) c - c/2 - (log amp)^2,  c = log(2 * 3.1415)
  dNLML/dtheta = -1/2 alpha^T dA alpha + 1/2 tr(A^-1 dA) + prior,  dA/damp = K,  dA/dnoise = I,  dA/dls = amp K o 2 D2 / ls
(D2: squared distances of the scaled rows), the prior term -2 log(amp) / amp for amp only, chained through softplus' = sigmoid.
"""
import numpy as np
from scipy.linalg import cho_solve, solve_triangular

LOG2PI = np.log(2. * 3.1415)  # the reference's literal, not pi


def softplus(x):
    return np.logaddexp(x, 0.)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def sqdist(x1, x2, ls):
    """Squared distances of x1 / ls and x2 / ls, the differences formed directly, summed over features in order."""
    a = np.asarray(x1, dtype=np.float64) / ls
    b = np.asarray(x2, dtype=np.float64) / ls
    d2 = np.zeros((a.shape[0], b.shape[0]))
    for k in range(a.shape[1]):
        t = a[:, k, None] - b[None, :, k]
        d2 += t * t
    return d2


def rbf(x1, x2, ls):
    return np.exp(-sqdist(x1, x2, ls))


class Oracle:
    def __init__(self, x, y):
        self.x = np.asarray(x, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64).ravel()
        self.ymean = np.mean(y)
        self.y = y - self.ymean
        self.n = self.x.shape[0]

    def factor(self, raw):
        amp, noise, ls = softplus(np.asarray(raw, dtype=np.float64))
        d2 = sqdist(self.x, self.x, ls)
        k = np.exp(-d2)
        a = amp * k + np.eye(self.n) * (noise + 1e-6)
        return amp, noise, ls, d2, k, a, np.linalg.cholesky(a)

    def evaluate(self, raw, with_grad=True):
        """(nlml, grad_raw or None, terms)"""
        raw = np.asarray(raw, dtype=np.float64)
        amp, noise, ls, d2, k, a, l = self.factor(raw)
        alpha = cho_solve((l, True), self.y)
        logdet_half = np.sum(np.log(np.diag(l)))
        nlml = 0.5 * self.y @ alpha + logdet_half + (self.n / 2.) * LOG2PI - 0.5 * LOG2PI - np.log(amp) ** 2
        terms = {"logdet_half": logdet_half, "y_ainv_y": self.y @ alpha}
        if not with_grad:
            return nlml, None, terms
        ainv = cho_solve((l, True), np.eye(self.n))
        kd = k * d2
        terms.update(a_k_a=alpha @ k @ alpha, tr_ainv_k=np.sum(ainv * k), a_kd_a=alpha @ kd @ alpha, tr_ainv_kd=np.sum(ainv * kd),
                     a_a=alpha @ alpha, tr_ainv=np.trace(ainv))
        quad = np.array([terms["a_k_a"], terms["a_a"], amp * 2.0 / ls * terms["a_kd_a"]])  # alpha^T dA alpha
        trace = np.array([terms["tr_ainv_k"], terms["tr_ainv"], amp * 2.0 / ls * terms["tr_ainv_kd"]])  # tr(A^-1 dA)
        g = -0.5 * quad + 0.5 * trace
        g[0] += -2.0 * np.log(amp) / amp
        terms["quad_half"] = 0.5 * quad
        terms["trace_half"] = 0.5 * trace
        return nlml, g * sigmoid(raw), terms

    def predict(self, raw, xt, full=False):
        amp, noise, ls, d2, k, a, l = self.factor(raw)
        alpha = cho_solve((l, True), self.y)
        cross = amp * rbf(self.x, xt, ls)  # [n, m]
        mean = cross.T @ alpha + self.ymean
        v = solve_triangular(l, cross, lower=True)
        if full:
            return mean.reshape(-1, 1), amp * rbf(xt, xt, ls) - v.T @ v
        return mean.reshape(-1, 1), amp - np.sum(v * v, axis=0)


def train(oracle, raw0=(0.0, -5.0, 0.0), steps=10, lr=0.01):
    """The reference loop restated with the oracle: raw parameters after each step and the NLML reported there."""
    raw = np.array(raw0, dtype=np.float64)
    m, s = np.zeros(3), np.ones(3)
    _, g, _ = oracle.evaluate(raw)
    traj, nlmls = [], []
    for i in range(steps):
        m = 0.9 * m + 0.1 * g
        s = 0.9 * s + 0.1 * g ** 2
        raw = raw - lr * m / np.sqrt(s + 1e-5)
        nlml, g, _ = oracle.evaluate(raw, i + 1 < steps)
        traj.append(raw.copy())
        nlmls.append(nlml)
    return traj, nlmls
