"""TEST INFRASTRUCTURE -- synthetic ProteinMPNN weights (no trained checkpoint is kept with the tests).

make_state_dict(seed, k) gives every parameter of the reference's vanilla ProteinMPNN (hidden 128, three encoder and three decoder
layers; state_dict keys and shapes as the reference's) from np.random.default_rng: matrices Xavier-scaled uniform, biases and the
LayerNorm weights and biases non-trivial, so that a dropped bias or affine term shows.  tools/make_golden_design.py and
tests/test_design.py both call it."""
import numpy as np
import torch

H = 128


def make_state_dict(seed, k=48):
    rng = np.random.default_rng([int(seed), int(k)])
    sd = {}

    def linear(name, n_out, n_in, bias=True):
        a = np.sqrt(6.0 / (n_in + n_out))
        sd[name + ".weight"] = rng.uniform(-a, a, (n_out, n_in))
        if bias:
            sd[name + ".bias"] = rng.uniform(-0.2, 0.2, n_out)

    def norm(name):
        sd[name + ".weight"] = 1.0 + rng.uniform(-0.3, 0.3, H)
        sd[name + ".bias"] = rng.uniform(-0.2, 0.2, H)

    linear("features.embeddings.linear", 16, 66)
    linear("features.edge_embedding", H, 416, bias=False)
    norm("features.norm_edges")
    linear("W_e", H, H)
    sd["W_s.weight"] = rng.normal(size=(21, H))
    for l in range(3):
        p = f"encoder_layers.{l}."
        for n in ("norm1", "norm2", "norm3"):
            norm(p + n)
        linear(p + "W1", H, 3 * H), linear(p + "W2", H, H), linear(p + "W3", H, H)
        linear(p + "W11", H, 3 * H), linear(p + "W12", H, H), linear(p + "W13", H, H)
        linear(p + "dense.W_in", 4 * H, H), linear(p + "dense.W_out", H, 4 * H)
    for l in range(3):
        p = f"decoder_layers.{l}."
        for n in ("norm1", "norm2"):
            norm(p + n)
        linear(p + "W1", H, 4 * H), linear(p + "W2", H, H), linear(p + "W3", H, H)
        linear(p + "dense.W_in", 4 * H, H), linear(p + "dense.W_out", H, 4 * H)
    linear("W_out", 21, H)
    return {k_: torch.tensor(v, dtype=torch.float32) for k_, v in sd.items()}
