import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scalable-meta-learning-with-gaussian-processes_amd")); sys.path.insert(0, ROOT)
import torch
from scamlgp_amd import ops
dev = torch.device("cuda:0")
torch.manual_seed(0)
for (T, N, D, kind) in [(512, 256, 8, 1), (512, 100, 3, 0), (1024, 48, 2, 1)]:
    X = torch.rand(T, N, D, dtype=torch.float64, device=dev)
    y = torch.randn(T, N, dtype=torch.float64, device=dev)
    theta = torch.cat([0.4 + torch.rand(T, D, dtype=torch.float64, device=dev), torch.ones(T, 1, dtype=torch.float64, device=dev),
                       torch.full((T, 1), 1e-3, dtype=torch.float64, device=dev)], 1)
    bad = torch.arange(T, device=dev) % 3 == 1
    theta[bad, D + 1] = -0.5          # indefinite: fails at some pivot, all retries fail too
    dup = torch.arange(T, device=dev) % 3 == 2
    X[dup, N // 2:] = X[dup, : N - N // 2]   # duplicated points + tiny negative noise: rescued by jitter
    theta[dup, D + 1] = -2e-9
    ref = None
    for rep in range(6):
        out = ops.gp_fit_fused(X, y, theta, kind)
        torch.cuda.synchronize()
        info, jit = out["info"].clone(), out["jitter"].clone()
        assert bool((info[bad] > 0).all()) and bool((info[~bad] == 0).all()), (info[:9], jit[:9])
        assert bool((jit[dup] > 0).all()) and bool((jit[~bad & ~dup] == 0).all())
        good = ~bad
        if ref is None:
            ref = (out["L"][good].clone(), info.clone(), jit.clone())
        else:
            assert torch.equal(out["L"][good], ref[0]) and torch.equal(info, ref[1]) and torch.equal(jit, ref[2])
    print(f"T={T} N={N}: {int(bad.sum())} failing, {int(dup.sum())} jitter-rescued ({sorted(set(jit[dup].tolist()))}), results stable over 6 runs", flush=True)
print("FAIL-PATH STRESS OK")
