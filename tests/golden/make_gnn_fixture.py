"""The `gnn_base.*` tensors of the reference's shipped checkpoints, as the fixture of the GNNBase tests (tests/gnn_lib.py):

    python tests/golden/make_gnn_fixture.py        # writes tests/golden/gnn_base.npz

Weights only — nothing of the reference runs here. Read: model_weights/tube/rot_inv/airtaxi/{actor,critic}.pt (F = 7: lin1 is (16, 9)) and
model_weights/tube/rotate/actor.pt (F = 8: lin1 is (16, 10)), under the reference root of ref_harness.REF. Stored as '<actor|critic|rotate>.<state-dict key>',
float32. The names and shapes pin the structure the restatement assumes: lin_key / lin_query / lin_value (48, 16) = three heads of 16; lin_edge (48, 1)
without bias; lin_skip (16, 16), so the heads are averaged before the skip; embed_layer.layer_norm and embed_layer.layers.2 are one LayerNorm stored twice.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as H  # noqa: E402

SOURCES = (("actor", "model_weights/tube/rot_inv/airtaxi/actor.pt"), ("critic", "model_weights/tube/rot_inv/airtaxi/critic.pt"),
           ("rotate", "model_weights/tube/rotate/actor.pt"))


def main():
    import torch
    out = {}
    for tag, rel in SOURCES:
        sd = torch.load(os.path.join(H.REF, rel), map_location="cpu")
        for k, v in sd.items():
            if k.startswith("gnn_base."):
                assert v.dtype == torch.float32, (k, v.dtype)
                out["%s.%s" % (tag, k)] = v.numpy()
        ln, dup = "gnn_base.gnn.embed_layer.layer_norm.", "gnn_base.gnn.embed_layer.layers.2."
        assert all(np.array_equal(out[tag + "." + ln + s], out[tag + "." + dup + s]) for s in ("weight", "bias")), tag
    path = os.path.join(HERE, "gnn_base.npz")
    np.savez_compressed(path, **out)
    print("%s: %d tensors, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
