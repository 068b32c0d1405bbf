"""Golden vectors for the policy's MLPBase (gmpe_mlp_forward / gmpe_mlp_backward), produced by RUNNING the reference on the CPU:

    python tests/golden/make_mlp_fixture.py        # writes tests/golden/mlp_base.npz

What runs (the reference's own code in float32; imports and stubs as in make_buffer_fixture.py): `MLPBase(args, (D,))` (onpolicy/algorithms/utils/mlp.py)
— the optional nn.LayerNorm(D), then MLPLayer's fc1 and layer_N copies of fc_h — with its parameters overwritten by the seeded draws of tests/mlp_lib.py,
on torch.cat of mlp_lib's seeded parts, and torch.autograd on loss = sum(features * gf) with respect to every part and every parameter.
Stored: outputs only (features, one gradient per part and per parameter, per case); the inputs are regenerated from their seeds by the tests.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_buffer_fixture as MB  # noqa: E402
import mlp_lib as M  # noqa: E402


def load_reference():
    MB.load_reference()
    from onpolicy.algorithms.utils.mlp import MLPBase
    return MLPBase


def module_params(base, case):
    """the module's parameters in mlp_lib.param_names order"""
    _, _, layer_n, _, fnorm = case
    ps = [base.feature_norm.weight, base.feature_norm.bias] if fnorm else []
    for seq in [base.mlp.fc1] + [base.mlp.fc2[i] for i in range(layer_n)]:
        ps += [seq[0].weight, seq[0].bias, seq[2].weight, seq[2].bias]
    return ps


def run_case(MLPBase, case):
    import torch
    rows, dims, layer_n, act, fnorm = case
    seed = M.seed_of(case)
    P, I = M.params(case, seed), M.inputs(case, seed)
    args = argparse.Namespace(use_feature_normalization=bool(fnorm), use_orthogonal=True, use_ReLU=act == "ReLU", stacked_frames=1, layer_N=layer_n,
                              hidden_size=M.H)
    base = MLPBase(args, (sum(dims),))
    ps = module_params(base, case)
    with torch.no_grad():
        for p, k in zip(ps, M.param_names(case)):
            p.copy_(torch.from_numpy(P[k]))
    assert type(base.mlp.fc1[1]).__name__ == act and base.mlp.fc1[2].eps == M.EPS and len(ps) == len(M.param_names(case))
    parts = [torch.from_numpy(a).requires_grad_() for a in M.split(I["x"], dims)]
    feats = base(torch.cat(parts, dim=1))
    assert tuple(feats.shape) == (rows, M.H)
    grads = torch.autograd.grad((feats * torch.from_numpy(I["gf"])).sum(), parts + ps)
    return dict(zip(M.out_names(case), [feats.detach().numpy()] + [g.numpy() for g in grads]))


def main():
    MLPBase = load_reference()
    import torch
    torch.set_num_threads(1)
    rec = {}
    for case in M.CASES:
        for k, v in run_case(MLPBase, case).items():
            rec["%s_%s" % (M.key(case), k)] = np.ascontiguousarray(v, np.float32)
    path = os.path.join(HERE, "mlp_base.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
