"""TEST INFRASTRUCTURE -- golden vectors for se3_diffusion_amd.design (fd_mpnn_graph, fd_mpnn_encoder, fd_mpnn_decode) from the
UNMODIFIED reference class ProteinMPNN (ProteinMPNN/protein_mpnn_utils.py) with the synthetic weights of tests/mpnn_weights.py
(make_state_dict(SEED, k), loaded with strict=True), on the CPU.

Run where the reference is present (oracle/ref_loader.py), in a process of its own:
    python tools/make_golden_design.py
Writes tests/golden/design.npz -- coordinates, random numbers and the reference's results: data only.

Per case (<name>_<key>):
  X, res_index, k        backbone N, CA, C, O float32 [L,4,3], residue numbers, k_neighbors
  E_idx                  features(...)'s neighbour table [L, min(k, L)]
  noise                  the randn of the decoding order, float32 [L]
  S_forced, order_forced, logp32, logp64
                         forward(..., use_input_decoding_order=True) on random letters, in float32 and after model.double()
  ref_gap                max |logp32 - logp64|
  fixed, S_true          positions that keep their letter (chain_M_pos = 1 - fixed) and the letters
  u, S, probs, order     sample(...) at T = 0.1, omit X, with torch.multinomial replaced IN THIS PROCESS by the inverse-CDF rule "the
                         first a with u < p_0 + .. + p_a" (float32 running sum) on the recorded uniforms u [L] (by position)
  logp_s32, score, global_score
                         forward on the sampled sequence with the sampled order, and the reference's _scores of it
  fasta                  (one case) the record protein_mpnn_run.py:367 writes, formatted here with the same expression

Two decision margins are ASSERTED, so that the tests' comparisons rest on conditions:
  (a) wherever L > k, every row's gap between the k-th and the (k+1)-th CA distance (float64) is >= 1e-4 A.  A synthetic chain
      that fails is redrawn (seed + 1000), a deposited chain's crop window moves on by one residue; `window` records the start.
  (b) at every sampling step the used u lies >= DELTA = 1e-3 inside its CDF interval; a u that does not is redrawn.

Cases: random-walk backbones of L = 1, 5, 17, 48, 49, 65 (ideal geometry, jittered: tools/make_golden_chain_batch.walk); walk17
has a jump of 40 in res_index, so both clip ends of the relative-position column are hit; walk17f = walk17's shape with a third of
its positions fixed; walk49k32 at k = 32; crops of 130 residues of the deposited chains 4GYT and 4YOW of
tests/golden/dssp_chains.npz.  k = 48 otherwise."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle import ref_loader as rl  # noqa: E402
from mpnn_weights import make_state_dict  # noqa: E402
from make_golden_chain_batch import walk  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "design.npz")
SEED = 20
DELTA = 1e-3
TEMP = 0.1
MARGIN_A = 1e-4
#        name         L    k   jump  fixed  source
CASES = (("walk1", 1, 48, False, False, None), ("walk5", 5, 48, False, False, None), ("walk17", 17, 48, True, False, None),
         ("walk17f", 17, 48, False, True, None), ("walk48", 48, 48, False, False, None), ("walk49", 49, 48, False, False, None),
         ("walk49k32", 49, 32, False, False, None), ("walk65", 65, 48, False, False, None),
         ("4GYT130", 130, 48, False, False, "4GYT"), ("4YOW130", 130, 48, False, False, "4YOW"))


def margin_a(X, k):
    ca = X[:, 1].astype(np.float64)
    if len(ca) <= k:
        return np.inf
    d = np.sort(np.sqrt(((ca[:, None] - ca[None]) ** 2).sum(-1) + 1e-6), -1)
    return float((d[:, k] - d[:, k - 1]).min())


def main():
    rl.install()
    sys.path.insert(0, os.path.join(rl.REF_ROOT, "ProteinMPNN"))
    import protein_mpnn_utils as pm

    dssp = np.load(os.path.join(ROOT, "tests", "golden", "dssp_chains.npz"))
    out = {"names": np.array([c[0] for c in CASES]), "delta": np.float64(DELTA), "temperature": np.float64(TEMP),
           "seed": np.int64(SEED)}
    models = {}
    for ci, (name, L, k, jump, fixed, src) in enumerate(CASES):
        if k not in models:
            m = pm.ProteinMPNN(num_letters=21, node_features=128, edge_features=128, hidden_dim=128, num_encoder_layers=3,
                               num_decoder_layers=3, augment_eps=0.0, k_neighbors=k)
            m.load_state_dict(make_state_dict(SEED, k), strict=True)
            m.eval()
            m64 = pm.ProteinMPNN(num_letters=21, node_features=128, edge_features=128, hidden_dim=128, num_encoder_layers=3,
                                 num_decoder_layers=3, augment_eps=0.0, k_neighbors=k)
            m64.load_state_dict(make_state_dict(SEED, k), strict=True)
            m64 = m64.double().eval()
            # (PositionalEncodings feeds its Linear a .float() one-hot: that Linear stays float32 -- a table lookup plus the bias,
            #  one float32 addition -- and everything behind it is float64 by promotion)
            m64.features.embeddings.linear.float()
            models[k] = (m, m64)
        model, model64 = models[k]
        rng = np.random.default_rng([SEED, ci])
        window = 0
        if src is None:
            while True:
                X = walk(np.random.default_rng([SEED, ci, window]), L)
                if margin_a(X, k) >= MARGIN_A:
                    break
                window += 1000
            ri = np.arange(L, dtype=np.int32)
            if jump:
                ri[L // 2:] += 40
        else:
            xyz, resnum = dssp[src + "_xyz"], dssp[src + "_resnum"]
            window = 10
            while margin_a(xyz[window:window + L], k) < MARGIN_A:
                window += 1
            X, ri = xyz[window:window + L].astype(np.float32), resnum[window:window + L].astype(np.int32)
        assert X.shape == (L, 4, 3) and margin_a(X, k) >= MARGIN_A
        fx = np.zeros(L, bool)
        if fixed:
            fx[rng.permutation(L)[:L // 3]] = True
        S_true = rng.integers(0, 20, L)
        noise = rng.standard_normal(L).astype(np.float32)

        Xt = torch.from_numpy(X)[None]
        ones = torch.ones(1, L)
        rit, enc = torch.from_numpy(ri.astype(np.int64))[None], torch.ones(1, L, dtype=torch.long)
        nz = torch.from_numpy(noise)[None]
        with torch.no_grad():
            _, E_idx = model.features(Xt, ones, rit, enc)
            # ---- forced ----
            S_forced = torch.from_numpy(rng.integers(0, 20, L))[None]
            order_f = torch.argsort((ones + 0.0001) * torch.abs(nz))
            lp32 = model(Xt, S_forced, ones, ones, rit, enc, nz, use_input_decoding_order=True, decoding_order=order_f)[0]
            lp64 = model64(Xt.double(), S_forced, ones.double(), ones.double(), rit, enc, nz.double(),
                           use_input_decoding_order=True, decoding_order=order_f)[0]
            # ---- sample ----
            used, worst = [], [np.inf]

            def inverse_cdf(probs, num_samples):
                assert num_samples == 1 and probs.shape == (1, 21)
                cdf = np.cumsum(probs[0].numpy().astype(np.float32), dtype=np.float32)
                while True:
                    u = np.float32(rng.uniform())
                    a = int(np.argmax(u < cdf)) if (u < cdf).any() else -1
                    lo = np.float32(0.0) if a <= 0 else cdf[a - 1]
                    if a >= 0 and u - lo >= DELTA and cdf[a] - u >= DELTA:
                        break
                used.append(u)
                worst[0] = min(worst[0], float(u - lo), float(cdf[a] - u))
                return torch.tensor([[a]], dtype=torch.int64)

            omit = np.zeros(21, np.float32)
            omit[20] = 1.0
            keep, torch.multinomial = torch.multinomial, inverse_cdf
            try:
                sd = model.sample(Xt, nz, torch.from_numpy(S_true)[None], ones, enc, rit, mask=ones, temperature=TEMP,
                                  omit_AAs_np=omit, bias_AAs_np=np.zeros(21, np.float32),
                                  chain_M_pos=torch.from_numpy((~fx).astype(np.float32))[None], omit_AA_mask=None,
                                  pssm_coef=None, pssm_bias=None, pssm_multi=0.0, pssm_log_odds_flag=False, pssm_log_odds_mask=None,
                                  pssm_bias_flag=False, bias_by_res=torch.zeros(1, L, 21))
            finally:
                torch.multinomial = keep
            order_s = sd["decoding_order"][0].numpy()
            assert len(used) == L and worst[0] >= DELTA * (1 - 1e-3)
            u = np.zeros(L, np.float32)
            u[order_s] = np.array(used, np.float32)
            chain_M = torch.from_numpy((~fx).astype(np.float32))[None]
            lps = model(Xt, sd["S"], ones, chain_M, rit, enc, nz, use_input_decoding_order=True,
                        decoding_order=sd["decoding_order"])
            score = pm._scores(sd["S"], lps, ones * chain_M)[0].numpy()
            gscore = pm._scores(sd["S"], lps, ones)[0].numpy()
        gap = float((lp32.double() - lp64).abs().max())
        rec = dict(X=X, res_index=ri, k=np.int64(k), window=np.int64(window), E_idx=E_idx[0].numpy().astype(np.int32), noise=noise,
                   S_forced=S_forced[0].numpy().astype(np.int64), order_forced=order_f[0].numpy().astype(np.int64),
                   logp32=lp32.numpy(), logp64=lp64.numpy(), ref_gap=np.float64(gap), fixed=fx, S_true=S_true.astype(np.int64), u=u,
                   S=sd["S"][0].numpy().astype(np.int64), probs=sd["probs"][0].numpy().astype(np.float32),
                   order=order_s.astype(np.int64), logp_s32=lps[0].numpy(), score=np.float32(score), global_score=np.float32(gscore))
        if fixed:
            S = sd["S"][0].numpy()
            seq = "".join("ACDEFGHIKLMNPQRSTVWYX"[a] for a in S)
            recov = torch.sum(torch.sum(torch.nn.functional.one_hot(torch.from_numpy(S_true), 21) *
                                        torch.nn.functional.one_hot(sd["S"][0], 21), axis=-1) * chain_M[0]) / torch.sum(chain_M[0])
            f = lambda v: np.format_float_positional(np.float32(v), unique=False, precision=4)
            rec["fasta"] = np.array(">T={}, sample={}, score={}, global_score={}, seq_recovery={}\n{}\n".format(
                TEMP, 1, f(score), f(gscore), f(recov.numpy()), seq))
        for key, v in rec.items():
            out[f"{name}_{key}"] = v
        print(f"{name}: L={L} k={k} window={window} margin_a={margin_a(X, k):.3g} ref_gap={gap:.3g} margin_b={worst[0]:.3g} "
              f"score={float(score):.4f}")
    np.savez_compressed(GOLD, **out)
    print("wrote", GOLD, os.path.getsize(GOLD), "bytes; max ref_gap",
          max(float(out[f"{c[0]}_ref_gap"]) for c in CASES))


if __name__ == "__main__":
    main()
