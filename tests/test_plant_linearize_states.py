"""The states that tests/test_gpu_plant_linearize.py and tests/test_gpu_tvlqr.py linearise about (tests/lin_cases.py: those of
tests/plant_cases.py, and fixed-seed ones for pendulum and free_body) meet their condition on the CPU: every one of the
1 + 6 nv perturbed host rollouts of 4 substeps ends with status 0 - no failed pivot, every state finite - which
lin_cases.host_linearize asserts column by column; and the host composition they give is finite.  No GPU."""
import numpy as np
import pytest

import lin_cases as lc


@pytest.mark.parametrize("name,S", [("pendulum", 3), ("acrobot", 3), ("hopper", 3), ("spinner", 3), ("free_body", 3), ("mini_cheetah", 2)])
def test_every_perturbed_host_rollout_ends_with_status_0(name, S):
    model = lc.case(name)[1]
    xn, A, B = lc.host_reference(name, S, 1e-3, 4)
    n = 2 * model.nv
    assert xn.shape == (S, model.nq + model.nv) and A.shape == (S, n, n) and B.shape == (S, n, model.nv)
    assert np.isfinite(xn).all() and np.isfinite(A).all() and np.isfinite(B).all()
