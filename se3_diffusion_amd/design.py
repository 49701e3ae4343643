"""Sequence design for backbones on the device: inference of the reference's vanilla (full-backbone) ProteinMPNN
(ProteinMPNN/protein_mpnn_utils.py:899-1168) on fd_mpnn_graph, fd_mpnn_encoder and fd_mpnn_decode (include/fd_hip.h).

One chain per backbone, every residue present, hidden size 128, three encoder and three decoder layers, k_neighbors from the
checkpoint.  Backbones of one call are packed, not padded: each is treated exactly as the reference treats it alone at
batch_size 1.  Not covered: ca_only, several chains, missing residues, tied_sample, PSSM inputs, bias_by_res,
conditional_probs / unconditional_probs, training.

The random numbers are this module's own: the decoding order is argsort((chain_mask + 1e-4) |order_noise|) as in the reference
(:1099), the letter of a step is drawn by inverse CDF from a uniform number -- not by the reference's torch.multinomial stream."""
from __future__ import annotations

import numpy as np
import torch

from . import hip

ALPHABET = "ACDEFGHIKLMNPQRSTVWYX"
H = 128
MAX_L = 1024                  # include/fd_hip.h FD_MPNN_MAX_L
MAX_K = 64                    # include/fd_hip.h FD_MPNN_MAX_K
NODE_SLOTS = 6                # include/fd_hip.h FD_MPNN_NODE_SLOTS
GRAPH_FLOATS = 71088          # include/fd_hip.h FD_MPNN_GRAPH_FLOATS
ENC_FLOATS = 991232           # include/fd_hip.h FD_MPNN_ENC_FLOATS
DEC_FLOATS = 654357           # include/fd_hip.h FD_MPNN_DEC_FLOATS


def _letters(x, what):
    """letters as int64 numpy: a string, a list of strings, or integers 0..20"""
    if isinstance(x, str):
        x = [x]
    if isinstance(x, (list, tuple)) and len(x) and isinstance(x[0], str):
        bad = [c for s in x for c in s if c not in ALPHABET]
        if bad:
            raise ValueError(f"{what}: letter {bad[0]!r} is not one of {ALPHABET}")
        if len({len(s) for s in x}) != 1:
            raise ValueError(f"{what}: strings of different length; pad with X")
        return np.array([[ALPHABET.index(c) for c in s] for s in x], np.int64)
    return None


class _Packer:
    """sd -> the three packed weight buffers of include/fd_hip.h"""

    def __init__(self, sd):
        self.sd = sd

    def __call__(self, key, shape=None):
        if key not in self.sd:
            raise ValueError(f"state_dict has no {key!r}")
        a = self.sd[key]
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        if shape is not None and tuple(a.shape) != tuple(shape):
            raise ValueError(f"{key}: shape {tuple(a.shape)}, expected {tuple(shape)} (only hidden_dim = node_features = "
                             f"edge_features = 128 is supported)")
        return a.astype(np.float32)

    def node_update(self, p):
        g = self
        return [g(p + "W3.weight", (H, H)).T, g(p + "W3.bias", (H,)), g(p + "norm1.weight", (H,)), g(p + "norm1.bias", (H,)),
                g(p + "dense.W_in.weight", (4 * H, H)).T, g(p + "dense.W_in.bias", (4 * H,)),
                g(p + "dense.W_out.weight", (H, 4 * H)).T, g(p + "dense.W_out.bias", (H,)),
                g(p + "norm2.weight", (H,)), g(p + "norm2.bias", (H,))]

    def graph(self):
        g = self
        mu = torch.linspace(2.0, 22.0, 16).numpy()
        pos = g("features.embeddings.linear.weight", (16, 66)).T + g("features.embeddings.linear.bias", (16,))[None]
        parts = [mu, pos, g("features.edge_embedding.weight", (H, 416)).T, g("features.norm_edges.weight", (H,)),
                 g("features.norm_edges.bias", (H,)), g("W_e.weight", (H, H)).T, g("W_e.bias", (H,))]
        return _flat(parts, GRAPH_FLOATS)

    def encoder(self):
        g = self
        parts = [g("encoder_layers.0.W1.bias", (H,))]
        dec_w1 = [g(f"decoder_layers.{m}.W1.weight", (H, 4 * H)) for m in range(3)]
        for l in range(3):
            p = f"encoder_layers.{l}."
            w1, w11 = g(p + "W1.weight", (H, 3 * H)), g(p + "W11.weight", (H, 3 * H))
            npw = np.zeros((H, NODE_SLOTS * H), np.float32)
            npb = np.zeros(NODE_SLOTS * H, np.float32)
            npw[:, 0:H], npw[:, H:2 * H] = w11[:, 0:H].T, w11[:, 2 * H:3 * H].T
            npb[0:H] = g(p + "W11.bias", (H,))
            if l < 2:
                nxt = g(f"encoder_layers.{l + 1}.W1.weight", (H, 3 * H))
                npw[:, 2 * H:3 * H], npw[:, 3 * H:4 * H] = nxt[:, 0:H].T, nxt[:, 2 * H:3 * H].T
                npb[2 * H:3 * H] = g(f"encoder_layers.{l + 1}.W1.bias", (H,))
            else:
                for m in range(3):
                    npw[:, (2 + m) * H:(3 + m) * H] = dec_w1[m][:, 3 * H:4 * H].T
                npw[:, 5 * H:6 * H] = dec_w1[0][:, 0:H].T
            parts += [w1[:, H:2 * H].T, g(p + "W2.weight", (H, H)).T, g(p + "W2.bias", (H,))] + self.node_update(p)
            parts += [npw, npb, w11[:, H:2 * H].T, g(p + "W12.weight", (H, H)).T, g(p + "W12.bias", (H,)),
                      g(p + "W13.weight", (H, H)).T, g(p + "W13.bias", (H,)), g(p + "norm3.weight", (H,)), g(p + "norm3.bias", (H,))]
        return _flat(parts, ENC_FLOATS)

    def decoder(self):
        g = self
        w1 = [g(f"decoder_layers.{l}.W1.weight", (H, 4 * H)) for l in range(3)]
        ws = g("W_s.weight", (21, H)).astype(np.float64)
        parts = [w[:, H:2 * H].T for w in w1] + [g(f"decoder_layers.{l}.W1.bias", (H,)) for l in range(3)]
        for l in range(3):
            p = f"decoder_layers.{l}."
            ts = (ws @ w1[l][:, 2 * H:3 * H].astype(np.float64).T).astype(np.float32)          # [21,128], rounded once
            parts += [w1[l][:, 0:H].T, w1[l][:, 3 * H:4 * H].T, ts, g(p + "W2.weight", (H, H)).T, g(p + "W2.bias", (H,))]
            parts += self.node_update(p)
        parts += [g("W_out.weight", (21, H)).T, g("W_out.bias", (21,))]
        return _flat(parts, DEC_FLOATS)


def _flat(parts, size):
    out = np.concatenate([np.ascontiguousarray(p, np.float32).reshape(-1) for p in parts])
    assert out.size == size, (out.size, size)
    return torch.from_numpy(out)


class SequenceDesigner:
    """ProteinMPNN inference on the device.  Build with from_state_dict / from_checkpoint; the packed weights and tables are
    prepared once here."""

    def __init__(self, gw, ew, dw, k_neighbors, device):
        if not 1 <= int(k_neighbors) <= MAX_K:
            raise ValueError(f"k_neighbors={k_neighbors}: expected 1..{MAX_K}")
        self.device = torch.device(device)
        self.k = int(k_neighbors)
        self.gw, self.ew, self.dw = (w.to(self.device).contiguous() for w in (gw, ew, dw))

    @classmethod
    def from_state_dict(cls, sd, k_neighbors=48, device=None):
        """sd: the reference model's own state_dict (features.embeddings.linear.*, features.edge_embedding.weight,
        features.norm_edges.*, W_e.*, W_s.weight, encoder_layers.{0,1,2}.*, decoder_layers.{0,1,2}.*, W_out.*)"""
        for k in sd:
            if k.startswith(("encoder_layers.3.", "decoder_layers.3.")):
                raise ValueError("only three encoder and three decoder layers are supported")
            if k.startswith("W_v."):
                raise ValueError("a ca_only checkpoint (W_v) is not supported")
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        pk = _Packer(sd)
        return cls(pk.graph(), pk.encoder(), pk.decoder(), k_neighbors, device)

    @classmethod
    def from_checkpoint(cls, path, device=None):
        """a checkpoint of the reference: a dict with 'model_state_dict' and 'num_edges'"""
        ck = torch.load(path, map_location="cpu")
        if not isinstance(ck, dict) or "model_state_dict" not in ck or "num_edges" not in ck:
            raise ValueError(f"{path}: expected a dict with 'model_state_dict' and 'num_edges'")
        return cls.from_state_dict(ck["model_state_dict"], k_neighbors=int(ck["num_edges"]), device=device)

    # -- inputs ------------------------------------------------------------------------------------------------------------------
    def prepare(self, atoms, lengths=None, residue_index=None):
        """Graph and encoder of the backbones, once: the result stands for `atoms` (with its lengths and residue_index) in any
        number of design() and score() calls."""
        pk = self._pack(atoms, lengths, residue_index)
        pk["enc"] = self.encode(pk)
        return pk

    def _pack(self, atoms, lengths, residue_index):
        """-> dict(atoms [T,4,3], res_index, offsets, chain_of, rows (flat b N + n of every packed row, or None), B, N, lens)"""
        if isinstance(atoms, dict) and "enc" in atoms:
            if lengths is not None or residue_index is not None:
                raise ValueError("prepared backbones carry their lengths and residue_index")
            return atoms
        dev = self.device
        x = torch.as_tensor(atoms)
        if x.dim() == 3:
            x = x[None]
        if x.dim() != 4 or x.shape[-1] != 3 or x.shape[-2] not in (4, 5, 37) or x.shape[1] < 1 or x.shape[0] < 1:
            raise ValueError(f"atoms: shape {tuple(torch.as_tensor(atoms).shape)}, expected [B,N,A,3] or [N,A,3] with A = 37 "
                             f"(atom37), 5 (N, CA, C, CB, O) or 4 (N, CA, C, O)")
        B, N, A = x.shape[:3]
        x = x.to(device=dev, dtype=torch.float32)
        if A != 4:
            x = x[:, :, [0, 1, 2, 4]]                     # atom37 and the sampler's five both keep O at 4
        if lengths is None:
            lens = [N] * B
        else:
            lens = [int(v) for v in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
            if len(lens) != B or min(lens) < 1 or max(lens) > N:
                raise ValueError(f"lengths: {B} values in 1..{N} expected")
        if max(lens) > MAX_L:
            raise ValueError(f"a backbone of {max(lens)} residues is above the kernels' limit of {MAX_L}")
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        T = int(off[-1])
        chain_of = np.repeat(np.arange(B, dtype=np.int32), lens)
        rows = None
        if lengths is not None and any(v != N for v in lens):
            rows = torch.from_numpy(np.concatenate([b * N + np.arange(v) for b, v in enumerate(lens)]).astype(np.int64)).to(dev)
        if residue_index is None:
            ri = torch.arange(N, dtype=torch.int32, device=dev)[None].expand(B, N)
        else:
            ri = torch.as_tensor(residue_index).to(device=dev, dtype=torch.int32)
            ri = ri[None] if ri.dim() == 1 else ri
            if tuple(ri.shape) != (B, N):
                raise ValueError(f"residue_index: shape {tuple(ri.shape)}, expected {(B, N)}")
        x, ri = x.reshape(B * N, 4, 3), ri.reshape(B * N)
        if rows is not None:
            x, ri = x.index_select(0, rows), ri.index_select(0, rows)
        return dict(atoms=x.contiguous(), res_index=ri.contiguous(), offsets=torch.from_numpy(off).to(dev),
                    chain_of=torch.from_numpy(chain_of).to(dev), rows=rows, B=B, N=N, T=T, lens=lens)

    def _to_packed(self, pk, x):
        """[B,S,N,...] -> [S,T,...]"""
        B, S, N = x.shape[:3]
        y = x.transpose(0, 1).reshape((S, B * N) + tuple(x.shape[3:]))
        return (y if pk["rows"] is None else y.index_select(1, pk["rows"])).contiguous()

    def _from_packed(self, pk, y, fill):
        """[S,T,...] -> [B,S,N,...], `fill` behind a backbone's length"""
        S, B, N = y.shape[0], pk["B"], pk["N"]
        if pk["rows"] is None:
            full = y
        else:
            full = torch.full((S, B * N) + tuple(y.shape[2:]), fill, dtype=y.dtype, device=y.device)
            full.index_copy_(1, pk["rows"], y)
        return full.reshape((S, B, N) + tuple(y.shape[2:])).transpose(0, 1).contiguous()

    # -- the three launches --------------------------------------------------------------------------------------------------------
    def graph(self, pk):
        """E_idx [T,K] int32 (positions within the backbone; -1 behind min(K, L)) and h_E [T,K,128]"""
        lib, dev, T, K = hip.get_lib(), self.device, pk["T"], self.k
        E_idx = torch.empty((T, K), dtype=torch.int32, device=dev)
        h_E = torch.empty((T, K, H), dtype=torch.float32, device=dev)
        lib.call("fd_mpnn_graph", pk["atoms"], pk["res_index"], pk["offsets"], pk["chain_of"], T, K, self.gw, E_idx, h_E)
        return E_idx, h_E

    def encode(self, pk):
        """graph + encoder of the packed backbones: one run serves every sequence of a backbone"""
        lib, dev, T, K = hip.get_lib(), self.device, pk["T"], self.k
        E_idx, h_E = self.graph(pk)
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        enc = dict(E_idx=E_idx, h_E=h_E, h_V=new(T, H), node=new(T, NODE_SLOTS, H), EB=new(3, T, K, H))
        lib.call("fd_mpnn_encoder", E_idx, pk["offsets"], pk["chain_of"], T, K, self.ew, self.dw, enc["h_V"], h_E, enc["node"],
                 new(T, NODE_SLOTS, H), enc["EB"])
        return enc

    def _decode(self, pk, enc, order, S_in, fixed, uniforms, omit, bias, temperature, forced):
        lib, dev, T = hip.get_lib(), self.device, pk["T"]
        S = order.shape[0]
        S_out = torch.empty((S, T), dtype=torch.int32, device=dev)
        log_probs = torch.empty((S, T, 21), dtype=torch.float32, device=dev)
        probs = torch.empty((S, T, 21), dtype=torch.float32, device=dev)
        scratch = torch.empty((S, T, 2, H), dtype=torch.float32, device=dev)
        lib.call("fd_mpnn_decode", enc["E_idx"], pk["offsets"], pk["B"], T, self.k, S, self.dw, enc["h_V"], enc["node"], enc["EB"],
                 order, S_in, fixed, uniforms, omit, bias, float(temperature), int(forced), scratch, S_out, log_probs, probs)
        return S_out, log_probs, probs

    # -- helpers -----------------------------------------------------------------------------------------------------------------
    def _order(self, pk, order_noise, chain_mask, S, generator):
        """decoding_order [B,S,N] int64 = argsort((chain_mask + 1e-4) |noise|) over each backbone's own residues (:1099)"""
        dev, B, N = self.device, pk["B"], pk["N"]
        if order_noise is None:
            order_noise = torch.randn((B, S, N), generator=generator, device=dev, dtype=torch.float32)
        else:
            order_noise = torch.as_tensor(order_noise).to(device=dev, dtype=torch.float32)
            if order_noise.dim() == 2 and B == 1:
                order_noise = order_noise[None]
            if tuple(order_noise.shape) != (B, S, N):
                raise ValueError(f"order_noise: shape {tuple(order_noise.shape)}, expected {(B, S, N)}")
        key = (chain_mask[:, None, :] + 0.0001) * order_noise.abs()
        if pk["rows"] is not None:
            beyond = torch.arange(N, device=dev)[None] >= torch.tensor(pk["lens"], device=dev)[:, None]
            key = key.masked_fill(beyond[:, None, :], float("inf"))
        return torch.argsort(key, dim=-1, stable=True)

    def _vec21(self, x, what):
        if x is None:
            return torch.zeros(21, dtype=torch.float32, device=self.device)
        if isinstance(x, str):
            v = np.zeros(21, np.float32)
            for c in x:
                if c not in ALPHABET:
                    raise ValueError(f"{what}: letter {c!r} is not one of {ALPHABET}")
                v[ALPHABET.index(c)] = 1.0
            return torch.from_numpy(v).to(self.device)
        v = torch.as_tensor(x).to(device=self.device, dtype=torch.float32).reshape(-1)
        if v.numel() != 21:
            raise ValueError(f"{what}: 21 values expected, in the order {ALPHABET}")
        return v.contiguous()

    def _seq_tensor(self, pk, seq, what, S=None):
        """letters [B,N] (or [B,S,N] when S is given) as int32 on the device"""
        dev, B, N = self.device, pk["B"], pk["N"]
        a = _letters(seq, what)
        t = torch.from_numpy(a) if a is not None else torch.as_tensor(seq)
        t = t.to(device=dev, dtype=torch.int32)
        want = (B, N) if S is None else (B, S, N)
        if t.dim() == 1 and B == 1:
            t = t[None]
        if S is not None and t.dim() == 2 and t.shape[0] == B:
            t = t[:, None, :].expand(B, S, t.shape[-1])
        if tuple(t.shape) != want:
            raise ValueError(f"{what}: shape {tuple(t.shape)}, expected {want}")
        return t.clamp(0, 20)

    def _result(self, pk, S_out, log_probs, probs, order, designed):
        S = self._from_packed(pk, S_out.to(torch.int64), 20)
        lp = self._from_packed(pk, log_probs, 0.0)
        nll = -lp.gather(-1, S[..., None])[..., 0]                                       # [B,S,N], zero behind the length
        lens = torch.tensor(pk["lens"], dtype=torch.float32, device=self.device)[:, None]
        out = dict(S=S, score=nll.sum(-1) / lens, log_probs=lp, probs=self._from_packed(pk, probs, 0.0), decoding_order=order,
                   lengths=list(pk["lens"]))
        if designed is not None:
            d = designed[:, None, :].to(torch.float32)
            out["score_designed"] = (nll * d).sum(-1) / d.sum(-1)
        else:
            out["score_designed"] = out["score"]
        out["designed"] = designed
        # (the one read-back, behind everything else)
        host = S.cpu().numpy()
        out["seqs"] = [["".join(ALPHABET[a] for a in host[b, s, :pk["lens"][b]]) for s in range(host.shape[1])]
                       for b in range(host.shape[0])]
        return out

    # -- public ------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def design(self, atoms, lengths=None, num_seqs=8, temperature=0.1, omit="X", bias=None, fixed=None, fixed_seq=None,
               generator=None, order_noise=None, uniforms=None, residue_index=None):
        """Sample num_seqs sequences for every backbone.

        atoms [B,N,37,3], [B,N,5,3] (N, CA, C, CB, O: the sampler's) or [B,N,4,3] (N, CA, C, O), or one backbone without B.
        lengths: host integers, the residues of each backbone in use.  omit: letters never drawn (a string, or 21 flags in the
        order ACDEFGHIKLMNPQRSTVWYX); bias: 21 values added to the logits.  fixed [B,N] (bool) with fixed_seq [B,N] (letters or
        strings): positions that keep their letter; they are decoded first and report probs = 0.  order_noise [B,num_seqs,N] and
        uniforms [B,num_seqs,N] replace the draws from `generator`.  residue_index [B,N]: residue numbers (default 0..N-1).

        Returns dict(S [B,num_seqs,N] int64 (X behind a backbone's length), seqs (strings, [B][num_seqs]), score [B,num_seqs] =
        mean of -log_probs[S] over the backbone (the reference's global_score), score_designed (over the positions that are not
        fixed: its score), log_probs and probs [B,num_seqs,N,21], decoding_order [B,num_seqs,N], lengths)."""
        if int(num_seqs) < 1:
            raise ValueError("num_seqs must be at least 1")
        if not float(temperature) > 0.0:
            raise ValueError("temperature must be positive")
        pk = self._pack(atoms, lengths, residue_index)
        dev, B, N, S = self.device, pk["B"], pk["N"], int(num_seqs)
        omit_v, bias_v = self._vec21(omit, "omit"), self._vec21(bias, "bias")
        fixed_t = S_in = fixed_rows = None
        chain_mask = torch.ones((B, N), dtype=torch.float32, device=dev)
        if fixed is not None:
            if fixed_seq is None:
                raise ValueError("fixed positions need fixed_seq")
            fixed_t = torch.as_tensor(fixed).to(device=dev)
            fixed_t = fixed_t[None] if fixed_t.dim() == 1 else fixed_t
            if tuple(fixed_t.shape) != (B, N):
                raise ValueError(f"fixed: shape {tuple(fixed_t.shape)}, expected {(B, N)}")
            fixed_t = fixed_t != 0
            chain_mask = (~fixed_t).to(torch.float32)
            S_in = self._to_packed(pk, self._seq_tensor(pk, fixed_seq, "fixed_seq", S))
            fixed_rows = self._to_packed(pk, fixed_t.to(torch.uint8)[:, None, :])[0].contiguous()
        order = self._order(pk, order_noise, chain_mask, S, generator)
        if uniforms is None:
            uniforms = torch.rand((B, S, N), generator=generator, device=dev, dtype=torch.float32)
        else:
            uniforms = torch.as_tensor(uniforms).to(device=dev, dtype=torch.float32)
            if uniforms.dim() == 2 and B == 1:
                uniforms = uniforms[None]
            if tuple(uniforms.shape) != (B, S, N):
                raise ValueError(f"uniforms: shape {tuple(uniforms.shape)}, expected {(B, S, N)}")
        enc = pk["enc"] if "enc" in pk else self.encode(pk)
        S_out, log_probs, probs = self._decode(pk, enc, self._to_packed(pk, order.to(torch.int32)), S_in, fixed_rows,
                                               self._to_packed(pk, uniforms), omit_v, bias_v, temperature, False)
        return self._result(pk, S_out, log_probs, probs, order, None if fixed_t is None else ~fixed_t)

    @torch.no_grad()
    def score(self, atoms, S, lengths=None, decoding_order=None, order_noise=None, generator=None, residue_index=None):
        """log_probs of given sequences S [B,num_seqs,N] (or [B,N]; letters or strings per backbone) under a decoding order:
        the reference's forward(use_input_decoding_order=True).  The order is decoding_order [B,num_seqs,N], or the argsort of
        |order_noise|, or drawn from `generator`.  Returns what design returns; probs is the softmax at temperature 1."""
        pk = self._pack(atoms, lengths, residue_index)
        dev, B, N = self.device, pk["B"], pk["N"]
        if isinstance(S, (list, tuple)) and len(S) and isinstance(S[0], (list, tuple)):
            S = np.stack([_letters(list(s), "S") for s in S])
        as_letters = _letters(S, "S")
        t = torch.as_tensor(S if as_letters is None else as_letters)
        if t.dim() == 1:
            t = t[None]
        if t.dim() == 2:
            t = t[:, None, :]
        if t.dim() != 3 or t.shape[0] != B or t.shape[2] != N:
            raise ValueError(f"S: shape {tuple(t.shape)}, expected [{B},num_seqs,{N}]")
        nS = t.shape[1]
        S_t = t.to(device=dev, dtype=torch.int32).clamp(0, 20)
        if decoding_order is not None:
            order = torch.as_tensor(decoding_order).to(device=dev, dtype=torch.int64)
            if order.dim() == 2 and B == 1:
                order = order[None]
            if tuple(order.shape) != (B, nS, N):
                raise ValueError(f"decoding_order: shape {tuple(order.shape)}, expected {(B, nS, N)}")
        else:
            order = self._order(pk, order_noise, torch.ones((B, N), dtype=torch.float32, device=dev), nS, generator)
        enc = pk["enc"] if "enc" in pk else self.encode(pk)
        zeros = torch.zeros(21, dtype=torch.float32, device=dev)
        S_out, log_probs, probs = self._decode(pk, enc, self._to_packed(pk, order.to(torch.int32)), self._to_packed(pk, S_t), None,
                                               None, zeros, zeros, 1.0, True)
        return self._result(pk, S_out, log_probs, probs, order, None)

    @staticmethod
    def fasta(name, out, temperature, backbone=0, native=None):
        """The records protein_mpnn_run.py:367 writes for the sequences of one backbone of a design() result:
        '>T=.., sample=.., score=.., global_score=.., seq_recovery=..' and the sequence, with the reference's
        np.format_float_positional(np.float32(.), unique=False, precision=4).  `name` labels the record set for the caller (the
        reference puts it on the native's record only, :348); native: the sequence seq_recovery compares with (letters or a
        string; default poly-alanine)."""
        del name
        b = int(backbone)
        L = out["lengths"][b]
        S = out["S"][b].cpu().numpy()[:, :L]
        nat = np.zeros(L, np.int64) if native is None else (_letters(native, "native")[0] if isinstance(native, str)
                                                            else np.asarray(native, np.int64))[:L]
        des = np.ones(L, bool) if out.get("designed") is None else out["designed"][b].cpu().numpy()[:L]
        score, glob = out["score_designed"][b].cpu().numpy(), out["score"][b].cpu().numpy()
        fmt = lambda v: np.format_float_positional(np.float32(v), unique=False, precision=4)
        text = ""
        for s in range(S.shape[0]):
            rec = np.float32(((S[s] == nat) & des).sum()) / np.float32(des.sum())
            text += ">T={}, sample={}, score={}, global_score={}, seq_recovery={}\n{}\n".format(
                temperature, s + 1, fmt(score[s]), fmt(glob[s]), fmt(rec), out["seqs"][b][s])
        return text
