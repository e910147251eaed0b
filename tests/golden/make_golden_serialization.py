"""Serialization codes and state_dict layout from the IMPORTED reference (build container only):

    python tests/golden/make_golden_serialization.py   ->  tests/golden/serialization_layout.npz

Data only, for tests/test_oracle_vs_reference.py: the reference's `encode` of seeded grids at every depth and order the
tests use (the inputs are rebuilt from the same seeds there), its `decode` of depth-9 Hilbert codes, and the names and
shapes of the reference policy's state_dict for the v1 and tiny variants."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

DEPTHS = (1, 3, 7, 8, 9, 12, 16)
ORDERS = ("z", "z-trans", "hilbert", "hilbert-trans")


def encode_inputs():
    """(depth, grid, batch) in the order the encode test draws them."""
    rng = np.random.default_rng(0)
    for depth in DEPTHS:
        g = rng.integers(0, 2 ** depth, size=(3000, 3)).astype(np.int32)
        b = rng.integers(0, 17, size=3000).astype(np.int64)
        yield depth, g, b


def hilbert_inputs():
    rng = np.random.default_rng(1)
    g = rng.integers(0, 2 ** 9, size=(2000, 3)).astype(np.int32)
    b = rng.integers(0, 4, size=2000).astype(np.int64)
    return g, b


def main():
    import ref_harness as rh

    rh.install_shims()
    from genrobo3d.models.PointTransformerV3.serialization import decode, encode

    out = {}
    for depth, g, b in encode_inputs():
        for o in ORDERS:
            out[f"encode_{depth}_{o}"] = encode(torch.from_numpy(g), torch.from_numpy(b), depth, o).numpy()
    g, b = hilbert_inputs()
    code = encode(torch.from_numpy(g), torch.from_numpy(b), 9, "hilbert")
    gc, bb = decode(code, 9, "hilbert")
    out.update(hilbert_code=code.numpy(), hilbert_decoded_grid=gc.numpy(), hilbert_decoded_batch=bb.numpy())
    for variant in ("v1", "tiny"):
        ref, _ = rh.build_reference_policy(variant)
        sd = ref.state_dict()
        out[f"layout_{variant}_names"] = np.array(list(sd))
        out[f"layout_{variant}_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
    path = os.path.join(HERE, "serialization_layout.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1e3:.0f} kB, {len(out)} arrays")


if __name__ == "__main__":
    main()
