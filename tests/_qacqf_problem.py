"""A small meta-learning problem for the joint q-point acquisition tests, stated twice from the same tensors: on the CPU through the
oracle (source fits, weighted prior, target posterior, Cholesky, Monte-Carlo value, torch autograd), and as a ScaMLGP model on the
GPU.  The CPU half needs no GPU, so the seeds are picked where the reference is computed.  Test infrastructure."""
import math

import torch

from oracle import gp_oracle as O
from tests import _qacqf_ref as R


class JointProblem:
    """T source tasks of ns[t] points (ragged where they differ), one weight pruned, n target points, B batches of q query points."""

    def __init__(self, ns, D, n, B, q, kind_s, kind_t, seed, ls_t=0.35):
        g = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.rand(*s, dtype=torch.float64, generator=g)        # noqa: E731
        nrm = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)      # noqa: E731
        T = len(ns)
        self.ns, self.T, self.D, self.n, self.B, self.q, self.kind_s, self.kind_t = list(ns), T, D, n, B, q, kind_s, kind_t
        sd = math.sqrt(D)
        self.Xs = [rnd(k, D) for k in ns]
        self.Ys = [(torch.sin(3.0 * x.sum(-1) / sd + t) + 0.1 * nrm(x.shape[0])).unsqueeze(-1) for t, x in enumerate(self.Xs)]
        self.theta_s = torch.cat([(0.4 + 0.4 * rnd(T, D)) * sd, 0.5 + rnd(T, 1), 1e-3 + 5e-3 * rnd(T, 1)], 1)   # (inside the source GPs' noise interval, 1e-8 .. 1e-2)
        self.Xt = rnd(n, D)
        self.yt = (torch.sin(3.0 * self.Xt.sum(-1) / sd + 0.5) + 0.3 * nrm(n)).unsqueeze(-1)
        self.w = 0.2 + 0.3 * rnd(T)
        self.w[1] = 1e-9   # pruned
        self.X = rnd(B, q, D)
        self.theta_t = torch.cat([torch.full((D,), ls_t * sd, dtype=torch.float64), torch.tensor([1.0, 5e-3], dtype=torch.float64)])
        self.m_all, self.s_all = (float(v) for v in self._standardiser())

    def _standardiser(self):
        Y = torch.cat(self.Ys + [self.yt], 0)
        m, s = Y.mean(0), (Y.std(0) if Y.shape[0] > 1 else torch.ones(1, dtype=torch.float64))
        return m.squeeze(), s.squeeze()

    # ---- the CPU statement ------------------------------------------------------------------------------------------------------
    def _source_fits(self):
        if not hasattr(self, "_fits"):
            self._fits = []
            for t in range(self.T):
                y = self.Ys[t].squeeze(-1)
                ym, ys = float(y.mean()), float(y.std())
                self._fits.append((O.gp_fit(self.Xs[t], (y - ym) / ys, self.theta_s[t], self.kind_s), ym, ys))
        return self._fits

    def joint_posterior(self, Xb):
        """mu (q,), Sigma (q, q) of one batch Xb (q, D) through the oracle, differentiable in Xb."""
        fits = self._source_fits()
        ystd = torch.tensor([f[2] for f in fits], dtype=torch.float64)
        mask = O.significant_weights_mask(self.w, ystd, 1e-3)
        assert not bool(mask[1]) and int(mask.sum()) == self.T - 1   # (the pruned weight is pruned, the others are not)
        xall = torch.cat([self.Xt, Xb])
        mus, covs = [], []
        for t in range(self.T):
            if bool(mask[t]):
                f, ym, ys = fits[t]
                mu, cov = O.source_posterior(xall, self.Xs[t], self.theta_s[t], self.kind_s, f["L"], f["alpha"], ym, ys, full_cov=True)
                mus.append(mu)
                covs.append(cov)
        mu_j, cov_j = O.target_prior(torch.stack(mus), torch.stack(covs), self.w[mask])
        return O.target_posterior(Xb, self.Xt, self.yt.squeeze(-1), mu_j, cov_j, self.theta_t, self.kind_t, self.m_all, self.s_all)

    def best_f(self):
        """qEI's incumbent for the comparisons: the mean of the target observations, in the bulk of the posterior, so that many samples
        improve and the gradient is live (the true incumbent, the minimum, leaves most samples at zero)."""
        return float(self.yt.mean())

    def reference(self, eps, acqf, par, jitters=None, check=True):
        """value (B,), grad (B, q, D) by autograd through the oracle; both conditions asserted on every batch."""
        X = self.X.clone().requires_grad_(True)
        vals = []
        for b in range(self.B):
            mu, Sigma = self.joint_posterior(X[b])
            jit = 0.0 if jitters is None else float(jitters[b])
            if check:
                R.assert_well_posed(mu.detach(), Sigma.detach(), eps, acqf, par, jit)
            vals.append(R.mc_value(mu, 0.5 * (Sigma + Sigma.T), eps, acqf, par, jit))
        v = torch.stack(vals)
        (g,) = torch.autograd.grad(v.sum(), X)
        return v.detach(), g

    # ---- the GPU statement ------------------------------------------------------------------------------------------------------
    def model(self, device):
        from scamlgp_amd import hyper, model as M
        stack = M.SourceGPStack([f"s{t}" for t in range(self.T)], self.Xs, self.Ys, kind=self.kind_s, device=device)
        stack.set_theta(self.theta_s)
        stack.refresh()
        gps = {tid: M.SourceGP(stack, i) for i, tid in enumerate(stack.task_ids)}
        base = (hyper.RBFKernel, hyper.MaternKernel)[self.kind_t]
        D = self.D
        cov = hyper.ScaleKernel(base(D, hyper.LogNormalPrior(0.5, 1.5), hyper.Interval(1e-4, 1e2), self.theta_t[:D]),
                                hyper.LogNormalPrior(-2.0, 3.0), hyper.Interval(1e-4, 1e2), float(self.theta_t[D]))
        lik = hyper.GaussianLikelihood(initial_value=float(self.theta_t[D + 1]))
        model = M.ScaMLGP(self.Xt, self.yt, gps, likelihood=lik, covar_module=cov).eval()
        model.weights = self.w.clone()
        return stack, model
