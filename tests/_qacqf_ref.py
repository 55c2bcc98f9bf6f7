"""The torch-fp64 statement of the joint Monte-Carlo acquisition (include/scaml_gp.h (7p)) that the CPU and GPU tests of qEI / qUCB
differentiate with autograd, and the two conditions under which a comparison with it means something.  Test infrastructure."""
import math

import torch

ACQF_UCB, ACQF_EI = 0, 1
LADDER = (0.0, 1e-8, 1e-7, 1e-6)
COND_MAX = 1e4       # cond(Sigma) of a compared batch
MARGIN = 1e-6        # a sample's distance from a tie and from a kink, in units of sqrt(max Sigma_jj)


def utilities(mu, Sigma, eps, acqf, par, jitter=0.0):
    """(S, q) utilities of the samples f_s = mu + C eps_s, C C^T = Sigma + jitter I, and C eps (S, q)."""
    q = Sigma.shape[-1]
    C = torch.linalg.cholesky(Sigma + jitter * torch.eye(q, dtype=Sigma.dtype))
    z = eps @ C.transpose(-1, -2)
    if acqf == ACQF_EI:
        return (par - (mu + z)).clamp_min(0.0), par - (mu + z), z
    return math.sqrt(par * math.pi / 2.0) * z.abs() - mu, z, z


def mc_value(mu, Sigma, eps, acqf, par, jitter=0.0):
    """value = (1/S) sum_s max_j utility_sj."""
    u, _, _ = utilities(mu, Sigma, eps, acqf, par, jitter)
    return u.max(-1).values.mean()


def semidefinite_cholesky(A):
    """The lower factor of a positive SEMI-definite matrix, the limit of cholesky(A + d I) as d -> 0+: a pivot that is zero to rounding
    (below 1e-12 of the largest diagonal entry, either sign) gives a zero column.  For a batch with two equal points, whose covariance is
    singular and whose last pivot comes out as +-1e-19 depending on the order of the sums that formed it."""
    q = A.shape[-1]
    C = torch.zeros_like(A)
    floor = 1e-12 * float(torch.diagonal(A).max())
    for k in range(q):
        piv = float(A[k, k] - (C[k, :k] ** 2).sum())
        if abs(piv) <= floor:
            continue
        C[k, k] = math.sqrt(piv)
        for i in range(k + 1, q):
            C[i, k] = (A[i, k] - (C[i, :k] * C[k, :k]).sum()) / C[k, k]
    return C


def mc_value_semidefinite(mu, Sigma, eps, par, jitter=0.0):
    """qEI's value with ``semidefinite_cholesky`` as the factor."""
    q = Sigma.shape[-1]
    z = eps @ semidefinite_cholesky(Sigma + jitter * torch.eye(q, dtype=Sigma.dtype)).T
    return (par - (mu + z)).clamp_min(0.0).max(-1).values.mean()


def assert_well_posed(mu, Sigma, eps, acqf, par, jitter=0.0):
    """Both conditions of the comparison, on the reference itself: cond(Sigma) <= 1e4, and every sample keeps 1e-6 sqrt(max Sigma_jj)
    between its winning and its runner-up entry and between every entry and its kink (0 of max(., 0) / |.|)."""
    with torch.no_grad():
        q = Sigma.shape[-1]
        S_ = Sigma + jitter * torch.eye(q, dtype=Sigma.dtype)
        ev = torch.linalg.eigvalsh(S_)
        assert ev[0] > 0 and ev[-1] / ev[0] <= COND_MAX, f"cond(Sigma) = {float(ev[-1] / ev[0]):.3g}"
        tol = MARGIN * math.sqrt(float(torch.diagonal(S_).max()))
        u, kink, _ = utilities(mu, S_, eps, acqf, par)
        assert float(kink.abs().min()) >= tol, "a sample sits on a kink"
        if q > 1:
            # (qEI: max_j max(g_j, 0) = max(max_j g_j, 0) -- the entries that compete are the g_j = best_f - f_j before the clamp; two
            #  clamped zeros are no tie, the sample's gradient is zero whichever of them "wins")
            top = torch.topk(kink if acqf == ACQF_EI else u, 2, dim=-1).values
            assert float((top[:, 0] - top[:, 1]).min()) >= tol, "a sample's two best entries tie"


def tail_reference(mu, Sigma, eps, acqf, par, jitter=0.0):
    """value, mubar = d value / d mu, Sigmabar = d value / d Sigma (symmetric) by autograd."""
    mu = mu.clone().requires_grad_(True)
    Sg = Sigma.clone().requires_grad_(True)
    v = mc_value(mu, 0.5 * (Sg + Sg.transpose(-1, -2)), eps, acqf, par, jitter)
    gm, gs = torch.autograd.grad(v, (mu, Sg))
    return v.detach(), gm, gs


def kernel(xa, xb, theta, kind):
    D = xa.shape[-1]
    d2 = (((xa.unsqueeze(-2) - xb.unsqueeze(-3)) / theta[:D]) ** 2).sum(-1)
    if kind == 0:
        return theta[D] * torch.exp(-0.5 * d2)
    r = torch.sqrt(d2.clamp_min(1e-30))
    return theta[D] * (1.0 + 5.0 ** 0.5 * r + (5.0 / 3.0) * r * r) * torch.exp(-(5.0 ** 0.5) * r)
