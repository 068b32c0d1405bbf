"""The heads' tensors of the reference's shipped checkpoints, as the fixture of the action-head and policy tests (tests/head_lib.py):

    python tests/golden/make_heads_fixture.py        # writes tests/golden/policy_heads.npz

Weights only — nothing of the reference runs here. Read, under the reference root of ref_harness.REF: act.action_out.linear.{weight,bias} of
model_weights/tube/rot_inv/airtaxi/actor.pt and model_weights/tube/rotate/actor.pt (both (25, 64) / (25,): 64 features, 25 actions), and
v_out.{weight,bias,stddev} of model_weights/tube/rot_inv/airtaxi/critic.pt, whichever of the three it holds (a PopArt v_out has all three, an nn.Linear
the first two). Stored as '<actor|rotate|critic>.<state-dict key>', float32.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as H  # noqa: E402

SOURCES = (("actor", "model_weights/tube/rot_inv/airtaxi/actor.pt", "act.action_out.linear.", ("weight", "bias")),
           ("rotate", "model_weights/tube/rotate/actor.pt", "act.action_out.linear.", ("weight", "bias")),
           ("critic", "model_weights/tube/rot_inv/airtaxi/critic.pt", "v_out.", ("weight", "bias", "stddev")))


def main():
    import torch
    out = {}
    for tag, rel, prefix, names in SOURCES:
        sd = torch.load(os.path.join(H.REF, rel), map_location="cpu")
        for n in names:
            if prefix + n in sd:
                v = sd[prefix + n]
                assert v.dtype == torch.float32, (tag, n, v.dtype)
                out["%s.%s%s" % (tag, prefix, n)] = v.numpy()
        assert "%s.%sweight" % (tag, prefix) in out and "%s.%sbias" % (tag, prefix) in out, tag
    path = os.path.join(HERE, "policy_heads.npz")
    np.savez_compressed(path, **out)
    print("%s: %d tensors, %d bytes" % (path, len(out), os.path.getsize(path)))
    for k, v in out.items():
        print("  %-40s %s" % (k, v.shape))


if __name__ == "__main__":
    main()
