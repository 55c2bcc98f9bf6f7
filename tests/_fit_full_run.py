"""What a GPU test needs to run one call through both instances of the N = 256 class of the fused fit: the switch between the
full-tile and the generic instance (the environment variable SCAML_FIT_NO_FULL, read by the launcher at every launch,
include/scaml_gp_debug.h), prefilled output buffers, the CU count the launcher's plan asks for.  For
tests/test_fit_full_build_gpu.py; a test module imports `switch` by name to use it as a fixture."""
import os

import pytest
import torch

N = 256
NO_FULL = "SCAML_FIT_NO_FULL"


@pytest.fixture
def switch():
    """switch(1): SCAML_FIT_NO_FULL set, the generic instance for every call; switch(0): unset, the choice by arguments.  The
    variable is put back to what it was when the test ends."""
    was = os.environ.get(NO_FULL)

    def set_mode(mode):
        if mode:
            os.environ[NO_FULL] = "1"
        else:
            os.environ.pop(NO_FULL, None)

    set_mode(0)
    yield set_mode
    if was is None:
        os.environ.pop(NO_FULL, None)
    else:
        os.environ[NO_FULL] = was


def cus(device):
    return torch.cuda.get_device_properties(device).multi_processor_count


def filled(T, device, store_L, want_linv, fill):
    """Output buffers for out=, L full of `fill` (what a call leaves alone must be the same in both runs)."""
    o = dict(L=torch.full((T, N, N), fill, dtype=torch.float64, device=device) if store_L else None,
             alpha=torch.zeros(T, N, dtype=torch.float64, device=device), info=torch.full((T,), -7, dtype=torch.int32, device=device),
             Linv_diag=torch.zeros(T, N // 16, 16, 16, dtype=torch.float64, device=device) if want_linv else None)
    o.update({k: torch.zeros(T, dtype=torch.float64, device=device) for k in ("quad", "logdet", "mll", "jitter")})
    return o
