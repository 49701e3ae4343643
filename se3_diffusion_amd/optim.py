"""Adam over flat buffers (fd_adam_step): the optimiser step of the training loop in one launch.

The reference trains with ``torch.optim.Adam(model.parameters(), lr=1e-4)`` (experiments/train_se3_diffusion.py:139);
over 282 parameter tensors that is 8 multi-tensor launches (0.76 ms of a 37 ms step on MI355X).  ``FlatAdam`` keeps
parameters, gradients and both moments in four flat fp32 buffers -- every ``p.data`` / ``p.grad`` is a view at a
256-byte offset (16-byte inside an ``adjacent`` group), so the GEMM kernels keep their 16-byte operand paths and the data-parallel all-reduce is one message -- and applies
the same update rule with one kernel.  ``state_dict`` / ``load_state_dict`` use torch.optim.Adam's layout, so
checkpoints written by either optimiser load into the other.

Guarded step (opt-in: ``max_grad_norm=`` and / or ``skip_nonfinite=True``): ``step()`` issues ``fd_adam_step_guarded``
instead -- gradient statistics, the decision and the update as three dependent launches.  The global L2 norm of ``flat_g``,
the clip coefficient ``min(1, max_grad_norm / (norm + 1e-6))`` (torch's ``clip_grad_norm_``), the count of non-finite
elements, the decision to skip, the count of applied steps and Adam's bias corrections all live in a small device state:
``step()`` reads nothing back, every data-parallel rank decides alike (take the step after the gradient all-reduce), and the
launches can be captured and replayed.  ``p.grad`` keeps the UNCLIPPED gradient -- unlike ``clip_grad_norm_`` the
coefficient is applied inside the update, not written back.  The norm is taken over the finite elements: with
``max_grad_norm`` alone (``skip_nonfinite=False``) a non-finite gradient element is not skipped and makes its own
parameter and moments non-finite (and only those).  ``health()`` returns the counters for a logger.

Moving average (opt-in: ``ema_decay=``): a fifth flat buffer ``ema`` holds an exponential moving average of the parameters,
the weights a diffusion model is sampled and evaluated from.  ``step()`` issues ``fd_adam_step_ema`` /
``fd_adam_step_guarded_ema`` instead: the same launches, whose update kernel ends with ``E += (1 - d_t) (P - E)`` on the
parameters it has just written (8 more bytes per parameter, no further launch).  ``d_t = ema_decay``, or with
``ema_warmup`` ``min(ema_decay, (1 + t) / (10 + t))`` with t the number of applied steps including this one.  A step the
guard skipped touches the average as little as the parameters, and does not advance the warm-up.  ``ema_weights()`` lets the
model compute with the average, ``ema_state_dict(model)`` / ``load_ema_state_dict(model, sd)`` carry it in a checkpoint of the
model's own keys; ``state_dict()`` stays torch.optim.Adam's layout and knows nothing of it.  Data parallel: nothing to add --
the update is elementwise and deterministic on identical parameters, so ranks that stepped on the same reduced gradient hold
the same average bit for bit.
"""
from __future__ import annotations

import contextlib

import torch
import torch.distributed as dist

from . import hip

_ALIGN = 64   # elements: 256-byte aligned views


class FlatAdam:
    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, adjacent=None, max_grad_norm=None,
                 skip_nonfinite=False, ema_decay=None, ema_warmup=True):
        """max_grad_norm: clip the gradient by its global L2 norm (None: no clipping; a value <= 0 is refused -- it would
        select the guarded step with clipping switched off, which nobody who writes 0 means); skip_nonfinite: leave parameters and
        moments untouched by a step whose gradient has an inf / NaN element.  Either one selects the guarded step (module
        docstring); with both at their defaults step() is the single fd_adam_step launch.  self.max_grad_norm, like self.lr,
        is passed by value at every step() and may be changed between steps (a captured step keeps the captured values).
        adjacent: groups (tuples) of parameters to lay out back to back without padding, in the given order, at the
        position of the group's first member (ScoreNetwork.flat_layout_groups(): weights that one kernel reads as one
        matrix, e.g. IPA's [linear_b ; down_z]).  The state_dict order stays that of `params`.
        ema_decay: keep a moving average of the parameters in self.ema (module docstring); None (default) allocates nothing and
        leaves step() the launches it has without it; a value outside (0, 1) is refused.  Like self.lr it is passed by value
        at every step() and may be changed between steps (not to None or from None: the buffer is allocated here).
        ema_warmup: d_t = min(ema_decay, (1 + t) / (10 + t)), so that the first steps do not average in the initial weights
        with the full decay."""
        self.params = [p for p in params if p.requires_grad]
        assert self.params, "no trainable parameters"
        assert all(p.dtype == torch.float32 for p in self.params), "fp32 parameters only"
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        dev = self.params[0].device
        group_of = {}
        for grp in (adjacent or ()):
            grp = [p for p in grp if p.requires_grad]
            assert all(p.numel() % 4 == 0 for p in grp[:-1]), "grouped parameters must keep their successors 16-byte aligned"
            for p in grp:
                group_of[id(p)] = grp
        placed, off = {}, 0
        for p in self.params:
            if id(p) in placed:
                continue
            for q in group_of.get(id(p), [p]):       # (a group is placed when its first member comes up)
                if id(q) in placed:
                    continue
                placed[id(q)] = off
                off += q.numel()
            off = (off + _ALIGN - 1) // _ALIGN * _ALIGN
        self.offsets = [placed[id(p)] for p in self.params]
        self.numel = off
        self.flat_p = torch.zeros(off, device=dev)
        self.flat_g = torch.zeros(off, device=dev)
        self.exp_avg = torch.zeros(off, device=dev)
        self.exp_avg_sq = torch.zeros(off, device=dev)
        for p, o in zip(self.params, self.offsets):
            view = self.flat_p[o:o + p.numel()].view_as(p)
            view.copy_(p.data)
            p.data = view
            p.grad = self.flat_g[o:o + p.numel()].view_as(p)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guarded = self.max_grad_norm is not None or self.skip_nonfinite
        self._max_norm_arg()     # (refuses max_grad_norm <= 0 here, not at the first step)
        self._t = 0              # steps taken by the unguarded step (property t); the guarded step counts on the device
        self._ws = self._opt_state = self._stats = None
        if self.guarded:         # (allocated here, not in step(): a captured step must not allocate)
            self._ws = torch.empty(hip.OPT_WS_DOUBLES, dtype=torch.float64, device=dev)
            self._opt_state = torch.zeros(hip.OPT_STATE_BYTES // 8, dtype=torch.int64, device=dev)
        self._dirty = False      # flat_g holds a gradient that step() / all_reduce_mean() already consumed (see rebind)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self.ema = None
        self._ema_live = False   # inside ema_weights(): flat_p holds the average, ema the training weights
        if self.ema_decay is not None:
            self._ema_decay_arg()                # (refuses a decay outside (0, 1) here, not at the first step)
            self.ema = self.flat_p.clone()       # (padding between the views is zero in both and stays zero)

    @property
    def t(self):
        """Steps taken, on the host: the unguarded step's count.  A guarded optimiser counts APPLIED steps on the device and
        has no host count that could go stale: applied_steps() / set_applied_steps()."""
        if self.guarded:
            raise AttributeError("a guarded FlatAdam counts its steps on the device: applied_steps() / set_applied_steps()")
        return self._t

    @t.setter
    def t(self, value):
        if self.guarded:
            raise AttributeError("a guarded FlatAdam counts its steps on the device: applied_steps() / set_applied_steps()")
        self._t = int(value)

    def _max_norm_arg(self):
        """max_norm of fd_adam_step_guarded (its "no clipping" is <= 0) from self.max_grad_norm (None: no clipping)"""
        if self.max_grad_norm is None:
            return 0.0
        if not self.max_grad_norm > 0.0:
            raise ValueError(f"max_grad_norm must be positive or None (no clipping), not {self.max_grad_norm!r}")
        return self.max_grad_norm

    def _ema_decay_arg(self):
        if not 0.0 < self.ema_decay < 1.0:
            raise ValueError(f"ema_decay must lie strictly between 0 and 1 (or be None: no average), not {self.ema_decay!r}")
        return self.ema_decay

    def rebind(self):
        """Make every p.data / p.grad a view of the flat buffers again.  Anything that replaces them behind the
        optimiser's back -- model.zero_grad() (set_to_none=True by default), module.to() / _apply -- would otherwise
        leave flat_g all-zero while autograd fills fresh tensors: the step would run on zeros without an error.
        A stray parameter value is copied into its view.  A stray gradient follows torch's semantics for a parameter
        whose .grad was None: the fresh tensor IS the gradient.  While the flat buffer still holds the gradient the last
        step() / all_reduce_mean() consumed (`_dirty`: nobody called zero_grad() on THIS object since -- the
        model.zero_grad()-only training loop), the stray gradient therefore REPLACES its view and a parameter left at
        .grad = None gets a zeroed view; after a zero_grad() it is added (nothing stale to overwrite, and a caller may
        have accumulated into the view before detaching it)."""
        bp, bg = self.flat_p.data_ptr(), self.flat_g.data_ptr()
        for p, o in zip(self.params, self.offsets):
            g = p.grad
            if p.data_ptr() == bp + 4 * o and g is not None and g.data_ptr() == bg + 4 * o:
                continue                                   # (the common case: two pointer reads per parameter)
            n = p.numel()
            if p.data.data_ptr() != self.flat_p.data_ptr() + 4 * o:
                view = self.flat_p[o:o + n].view_as(p)
                view.copy_(p.data)
                p.data = view
            if p.grad is None:
                view = self.flat_g[o:o + n].view_as(p)
                if self._dirty:
                    view.zero_()
                p.grad = view
            elif p.grad.data_ptr() != self.flat_g.data_ptr() + 4 * o:
                view = self.flat_g[o:o + n].view_as(p)
                if self._dirty:
                    view.copy_(p.grad.to(view.dtype))
                else:
                    view.add_(p.grad.to(view.dtype))
                p.grad = view

    # -- gradient buffer (dist.FlatGrads interface) ------------------------------------------------------------
    def zero_grad(self, set_to_none=False):
        self.flat_g.zero_()
        for p in self.params:          # a stray gradient (see rebind) is dropped with the rest
            if p.grad is not None and not (self.flat_g.data_ptr() <= p.grad.data_ptr() < self.flat_g.data_ptr() + 4 * self.numel):
                p.grad = None
        self._dirty = False
        self.rebind()

    zero = zero_grad

    def all_reduce_mean(self):
        self.rebind()
        if dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(self.flat_g, op=dist.ReduceOp.SUM)
            self.flat_g.div_(dist.get_world_size())
        self._dirty = True

    # -- update ------------------------------------------------------------------------------------------------------
    def step(self):
        if self._ema_live:
            raise RuntimeError("step() inside ema_weights(): the parameters are the average there, not the training weights")
        self.rebind()
        b1, b2 = self.betas
        if self.guarded:
            if self.ema is None:
                hip.get_lib().call("fd_adam_step_guarded", self.flat_p, self.flat_g, self.exp_avg, self.exp_avg_sq, self.numel,
                                   self.lr, b1, b2, self.eps, self._max_norm_arg(), int(self.skip_nonfinite), self._ws,
                                   self._opt_state)
            else:
                hip.get_lib().call("fd_adam_step_guarded_ema", self.flat_p, self.flat_g, self.exp_avg, self.exp_avg_sq, self.ema,
                                   self.numel, self.lr, b1, b2, self.eps, self._max_norm_arg(), int(self.skip_nonfinite),
                                   self._ws, self._opt_state, self._ema_decay_arg(), int(self.ema_warmup))
            self._dirty = True
            return
        if self.ema is None:
            self._t += 1
            hip.get_lib().call("fd_adam_step", self.flat_p, self.flat_g, self.exp_avg, self.exp_avg_sq, self.numel,
                               self.lr, b1, b2, self.eps, 1.0 - b1 ** self._t, 1.0 - b2 ** self._t)
        else:
            d = self._ema_decay_arg()            # (before the count advances: a refused decay takes no step)
            self._t += 1
            if self.ema_warmup:
                d = min(d, (1.0 + self._t) / (10.0 + self._t))
            hip.get_lib().call("fd_adam_step_ema", self.flat_p, self.flat_g, self.exp_avg, self.exp_avg_sq, self.ema, self.numel,
                               self.lr, b1, b2, self.eps, 1.0 - b1 ** self._t, 1.0 - b2 ** self._t, 1.0 - d)
        self._dirty = True

    # -- the moving average ------------------------------------------------------------------------------------------
    def _need_ema(self):
        if self.ema is None:
            raise RuntimeError("this FlatAdam keeps no moving average (ema_decay=None)")

    def _exchange_ema(self):
        tmp = self.flat_p.clone()
        self.flat_p.copy_(self.ema)
        self.ema.copy_(tmp)

    def reset_ema(self):
        """Average := the current parameters (after the model loaded a checkpoint that carries no average)."""
        self._need_ema()
        if self._ema_live:
            raise RuntimeError("reset_ema() inside ema_weights()")
        self.rebind()
        self.ema.copy_(self.flat_p)

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the context the model computes with the averaged weights; after it the training weights are back bit for
        bit, also when the body raises.  The CONTENTS of flat_p and ema are exchanged in place (copies through one temporary
        of the flat size), so every p.data stays a view of flat_p at its address and nothing that holds a parameter's address
        goes stale (dist.FlatGrads, a captured graph, the plane split of the weights, which is keyed by address).  step() and
        reset_ema() raise inside it, and it does not nest.
        Do NOT enter it between a training forward and its backward: the backward would read weights (and planes split from
        them) that are no longer the ones the forward used.  The training forward re-splits the weight planes at every step
        and a no-grad forward clears them, so the exchange is safe between steps and around sampling."""
        self._need_ema()
        if self._ema_live:
            raise RuntimeError("ema_weights() does not nest")
        self.rebind()
        self._exchange_ema()
        self._ema_live = True
        try:
            yield self
        finally:
            self._exchange_ema()
            self._ema_live = False

    def _ema_slices(self, model):
        """(key, view of self.ema) for every tensor of model.state_dict() that lives inside flat_p, found by address"""
        self.rebind()
        at = {self.flat_p.data_ptr() + 4 * o: (o, p.numel()) for p, o in zip(self.params, self.offsets)}
        out = []
        for k, t in model.state_dict().items():
            hit = at.get(t.data_ptr()) if t.dtype == torch.float32 and t.device == self.flat_p.device else None
            if hit is not None and hit[1] == t.numel():
                out.append((k, self.ema[hit[0]:hit[0] + hit[1]].view(t.shape)))
        return out

    def ema_state_dict(self, model):
        """model.state_dict() with every tensor that lives inside flat_p replaced by a clone of its slice of the average
        (buffers and frozen parameters are the model's own): the model's keys and shapes, so it loads with strict=True into a
        ScoreNetwork and into the reference's model -- the "model" entry of a second checkpoint for an unchanged inference
        script."""
        self._need_ema()
        if self._ema_live:
            raise RuntimeError("ema_state_dict() inside ema_weights(): model.state_dict() is the average there")
        sd = model.state_dict()
        for k, view in self._ema_slices(model):
            sd[k] = view.clone()
        return sd

    def load_ema_state_dict(self, model, sd):
        """The inverse of ema_state_dict: the average := the entries of sd that belong to tensors inside flat_p.  A missing
        key or a wrong shape is an error, and nothing is written then."""
        self._need_ema()
        if self._ema_live:
            raise RuntimeError("load_ema_state_dict() inside ema_weights()")
        slices = self._ema_slices(model)
        for k, view in slices:
            if k not in sd:
                raise KeyError(f"load_ema_state_dict: missing key {k!r}")
            if tuple(sd[k].shape) != tuple(view.shape):
                raise ValueError(f"load_ema_state_dict: {k!r} has shape {tuple(sd[k].shape)}, the model's is {tuple(view.shape)}")
        for k, view in slices:
            view.copy_(sd[k])

    # -- gradient health ---------------------------------------------------------------------------------------------
    def grad_stats(self, out=None):
        """fd_grad_stats of the current flat_g: a device tensor of 4 doubles {sum of squares over the finite elements, count of
        non-finite elements, max |g| over the finite ones, 0}; nothing is read back.  Without `out` the result is ONE tensor
        owned by the optimiser, allocated at the first call and overwritten by every later one (no allocation or fill per
        step; call once before capturing, or pass `out`: a contiguous float64 tensor of 4 elements on the buffer's device).
        In data-parallel training call it after all_reduce_mean() / OverlapAllReduce.finish(), so every rank sees the same
        figures."""
        self.rebind()
        if self._ws is None:
            self._ws = torch.empty(hip.OPT_WS_DOUBLES, dtype=torch.float64, device=self.flat_g.device)
        if out is None:
            if self._stats is None:
                self._stats = torch.zeros(4, dtype=torch.float64, device=self.flat_g.device)
            out = self._stats
        assert out.dtype == torch.float64 and out.numel() == 4 and out.is_contiguous(), "out: 4 contiguous doubles"
        hip.get_lib().call("fd_grad_stats", self.flat_g, self.numel, self._ws, out)
        return out

    def health(self):
        """The guarded step's device state as Python numbers, with ONE device-to-host copy (for a logger that calls it every k
        steps): step (applied steps), skipped, clipped (counters), and nonfinite, grad_norm, clip_coef, max_abs of the latest
        step() (grad_norm / max_abs over the finite elements; clip_coef = 1 for a skipped step)."""
        assert self.guarded, "health() reads the state of the guarded step (max_grad_norm= / skip_nonfinite=)"
        st = hip.FdOptState.from_buffer_copy(self._opt_state.cpu().numpy().tobytes())
        return {"step": int(st.step), "skipped": int(st.skipped), "clipped": int(st.clipped), "nonfinite": int(st.nonfinite),
                "grad_norm": float(st.grad_norm), "clip_coef": float(st.clip_coef), "max_abs": float(st.max_abs)}

    def applied_steps(self):
        """Adam's t: the device counter when guarded (one device-to-host copy), the host count otherwise."""
        return self.health()["step"] if self.guarded else self._t

    def set_applied_steps(self, t):
        """Set Adam's t (what load_state_dict does with a checkpoint's "step"): the device counter when guarded."""
        if self.guarded:
            self._opt_state[:1].fill_(int(t))      # (FdOptState.step)
        else:
            self._t = int(t)

    # -- torch.optim.Adam-compatible checkpoints (data/utils.py:353-362 saves optimizer.state_dict()) ----------------
    def state_dict(self):
        state = {}
        t = self.applied_steps()
        for i, (p, o) in enumerate(zip(self.params, self.offsets)):
            n = p.numel()
            state[i] = {"step": torch.tensor(float(t)),
                        "exp_avg": self.exp_avg[o:o + n].view_as(p).clone(),
                        "exp_avg_sq": self.exp_avg_sq[o:o + n].view_as(p).clone()}
        group = {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": 0, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "params": list(range(len(self.params)))}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        group = sd["param_groups"][0]
        self.lr, self.betas, self.eps = float(group["lr"]), tuple(float(b) for b in group["betas"]), float(group["eps"])
        assert not group.get("weight_decay", 0) and not group.get("amsgrad", False), "plain Adam only"
        t = None
        for i, (p, o) in enumerate(zip(self.params, self.offsets)):
            st = sd["state"].get(i)
            if st is None:
                continue
            n = p.numel()
            self.exp_avg[o:o + n].copy_(st["exp_avg"].reshape(-1))
            self.exp_avg_sq[o:o + n].copy_(st["exp_avg_sq"].reshape(-1))
            t = int(float(st["step"]))
        if t is not None:        # (a checkpoint without optimiser state leaves the count alone)
            self.set_applied_steps(t)
