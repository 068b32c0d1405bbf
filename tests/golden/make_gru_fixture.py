"""Golden vectors for the masked GRU layer (gmpe_gru_forward / gmpe_gru_backward), produced by RUNNING the reference on the CPU:

    python tests/golden/make_gru_fixture.py        # writes tests/golden/gru_layer_<pattern>.npz, one file per mask pattern

What runs (the reference's own code in float32; imports and stubs as in make_ppo_loss_fixture.py): `RNNLayer(64, 64, 1, True)`
(onpolicy/algorithms/utils/rnn.py) — nn.GRU driven by the segment loop, then nn.LayerNorm — with its parameters overwritten by the seeded draws of
tests/gru_lib.py, on gru_lib's seeded x, hxs and masks, and torch.autograd on loss = sum(features * gf) + sum(hxs_out * gh).
Stored: outputs only (features, hxs_out and the eight gradients per case); the inputs are regenerated from their seeds by the tests. One file per mask
pattern, because the four together (the weight gradients of sixteen runs) would pass the size limit of a committed file.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_buffer_fixture as MB  # noqa: E402
import gru_lib as G  # noqa: E402


def load_reference():
    MB.load_reference()
    from onpolicy.algorithms.utils.rnn import RNNLayer
    return RNNLayer


def run_case(RNNLayer, L, Nb, pattern):
    import torch
    P, I, m = G.params(), G.inputs(L, Nb), G.masks(L, Nb, pattern)
    layer = RNNLayer(G.D, G.H, 1, True)
    with torch.no_grad():
        for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            getattr(layer.rnn, k + "_l0").copy_(torch.from_numpy(P[k]))
        layer.norm.weight.copy_(torch.from_numpy(P["ln_weight"]))
        layer.norm.bias.copy_(torch.from_numpy(P["ln_bias"]))
    assert layer.norm.eps == G.EPS
    x, hxs = torch.from_numpy(I["x"]).requires_grad_(), torch.from_numpy(I["hxs"]).requires_grad_()
    feats, hout = layer(x, hxs, torch.from_numpy(m))
    assert tuple(feats.shape) == (L * Nb, G.H) and tuple(hout.shape) == (Nb, 1, G.H)
    loss = (feats * torch.from_numpy(I["gf"])).sum() + (hout * torch.from_numpy(I["gh"])).sum()
    ps = [layer.rnn.weight_ih_l0, layer.rnn.weight_hh_l0, layer.rnn.bias_ih_l0, layer.rnn.bias_hh_l0, layer.norm.weight, layer.norm.bias]
    grads = torch.autograd.grad(loss, [x, hxs] + ps, allow_unused=True)
    out = dict(features=feats.detach().numpy(), hxs_out=hout.detach().numpy())
    for k, g, like in zip(G.GRADS, grads, [x, hxs] + ps):
        out[k] = (torch.zeros_like(like) if g is None else g).numpy()
    return out


def main():
    RNNLayer = load_reference()
    import torch
    torch.set_num_threads(1)
    for pattern in G.PATTERNS:
        rec = {}
        for L, Nb in G.CASES:
            for k, v in run_case(RNNLayer, L, Nb, pattern).items():
                rec["%s_%s" % (G.key(L, Nb, pattern), k)] = np.ascontiguousarray(v, np.float32)
        path = os.path.join(HERE, "gru_layer_%s.npz" % pattern)
        np.savez_compressed(path, **rec)
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
