"""Fused multi-tensor optimisers: every parameter (and its gradient and optimiser state) lives in ONE flat fp32 buffer, so a
step is a single streaming kernel over 3-4 arrays and the data-parallel gradient exchange is a single RCCL all-reduce of one
contiguous 57 MB bucket (no per-tensor launches, no flatten/unflatten copies).

FusedOptimizer is the optimiser-independent half (bucket, prebuild, state files, device-resident step counter and learning rate);
FusedAdam, FusedSGD, FusedRMSprop and FusedAdagrad are the reference's `OPTIMIZATION.optimizer` choices (utils/training_utils.py:11-53)
behind it.  The step plan, the captured graphs, the all-reduce and the layout refresh use only step(), .flat, prebuild(),
sync_hyperparameters() and flat.touched(), so any of the four runs the online driver."""
import torch

from . import _lib as L


class FlatParams:
    """Re-homes a list of parameters into one contiguous, 16-byte aligned buffer (params become views) and keeps
    a matching flat gradient buffer whose slices are installed as `.grad`."""

    def __init__(self, params):
        params = [p for p in params]
        if not params:
            raise ValueError("no parameters")
        dev = params[0].device
        offs, total = [], 0
        for p in params:
            offs.append(total)
            total += (p.numel() + 3) // 4 * 4            # keep every slice 16-byte aligned
        self.params, self.offsets, self.numel = params, offs, total
        self.data = torch.zeros(total, device=dev, dtype=torch.float32)
        # gradients + a 16-byte tail whose first element counts the ranks that contributed to the bucket (dist.exchange_gradients_)
        self.grad_ext = torch.zeros(total + 4, device=dev, dtype=torch.float32)
        self.grad = self.grad_ext[:total]
        self.grad_ext[total] = 1.0
        with torch.no_grad():
            for p, o in zip(params, offs):
                self.data[o:o + p.numel()].copy_(p.reshape(-1))
                p.data = self.data[o:o + p.numel()].view_as(p)
        # state the convolution module path reads through the parameters (e2ehip.conv): a counter of raw-pointer rewrites of the
        # parameters (their torch version counters do not move), and the direct-gradient switch + side stream of direct_weight_grads()
        self.epoch = [1]
        self.direct, self.overlap, self.side = False, False, None
        self.bind_grads()

    def bind_grads(self):
        for p, o in zip(self.params, self.offsets):
            p.grad = self.grad[o:o + p.numel()].view_as(p)
            p._e2e_grad_sink = p.grad              # conv backward may accumulate straight into it (conv.direct_weight_grads)
            p._e2e_grad_owner = self
            p._e2e_epoch = self.epoch

    def touched(self):
        """The parameters were rewritten through raw pointers (optimiser kernel, broadcast): GEMM layouts cached on them are stale."""
        self.epoch[0] += 1

    def side_stream(self):
        if self.side is None:
            self.side = torch.cuda.Stream(self.data.device)
        return self.side

    def zero_grad(self):
        self.grad.zero_()
        self.bind_grads()

    def participants(self):
        return self.grad_ext[self.numel:self.numel + 1]


class FusedOptimizer(torch.optim.Optimizer):
    """What the fused optimisers share: ONE parameter group over ONE flat bucket.  Like torch, parameters whose gradient never appears
    are not moved: a parameter is only updated from the first step in which its gradient slice is non-None, and frozen parameters
    (requires_grad False) are skipped -- both are handled by an `active` mask folded into the flat layout (inactive parameters are simply
    left out of the flat buffer).  The step count and the learning rate live on the device, so a step can be captured into a hipGraph and
    replayed; the state is read and written in the corresponding torch optimiser's own state-dict format.

    A subclass names its state arrays (STATE), the group keys a loaded file may set (HYPER), refuses what its kernel does not implement
    (_refuse) and launches the kernel (_launch)."""

    STATE = ()                  # ((key in torch's per-parameter state, attribute holding the flat array), ...)
    HYPER = ("lr",)             # hyper-parameters of the group: named in the one-group message, taken over from a loaded file
    STEP_IN_STATE = True        # torch's per-parameter state carries "step"
    STEP_IN_UPDATE = False      # ... and the update depends on it (Adam's bias corrections): one counter must fit every parameter

    def __init__(self, params, defaults):
        super().__init__(list(params), defaults)
        if len(self.param_groups) != 1:
            raise NotImplementedError(self._one_group())
        self._refuse(self.param_groups[0])
        self._all = list(self.param_groups[0]["params"])
        self._pending = None
        self._loaded = False
        self.flat = None
        self.steps = 0              # host-side count of step() CALLS; the step that counts lives on the device (graph replays)
        self._counter = self._lr = self._hyper_key = None

    def _one_group(self):
        return f"{type(self).__name__} steps ONE parameter group (one {' / '.join(self.HYPER)} for the flat bucket)"

    def _refuse(self, group):
        """NotImplementedError naming the option when `group` (this optimiser's own, or a loaded file's) asks for one the kernel lacks."""

    def _launch(self, group):
        raise NotImplementedError

    # ---- device-resident scalars ----------------------------------------------------------------------------------------------------
    def _resident_state(self):
        """Device-resident step counter (1-based: steps done + 1) and learning rate; the rate is rewritten IN PLACE when the group's
        changed, so a captured launch that is replayed afterwards reads the new one."""
        lr = float(self.param_groups[0]["lr"])
        if self._counter is None:
            dev = self.flat.data.device
            self._counter = torch.ones(1, device=dev, dtype=torch.int32)
            self._lr = torch.empty(1, device=dev, dtype=torch.float32)
        if self._hyper_key != lr:
            self._lr.fill_(lr)
            self._hyper_key = lr
        return self._lr, self._counter

    def sync_hyperparameters(self):
        """Bring what the device holds in line with param_groups[0] -- the learning rate; for Adam the table built from lr and betas --
        touching device memory only on a change.  step() calls it; whoever REPLAYS a captured step() calls it on the host before the
        replay (RefineStepPlan.step / idle_step), which is how a learning-rate scheduler stepped between two refinement steps reaches
        a graph that was captured under the old rate.  Before the bucket exists there is nothing to bring in line."""
        if self.flat is not None:
            self._resident_state()

    def steps_done(self):
        """Optimiser steps taken so far, read from the device counter (host sync)."""
        return 0 if self._counter is None else int(self._counter.item()) - 1

    # ---- the flat layout ------------------------------------------------------------------------------------------------------------
    def _adopt(self, act):
        self.flat = FlatParams(act)
        for _, attr in self.STATE:
            setattr(self, attr, torch.zeros_like(self.flat.data))

    def _build(self):
        # parameters that take part: trainable AND with a gradient at the first step (torch skips grad None)
        act = [p for p in self._all if p.requires_grad and p.grad is not None]
        if not act:
            raise RuntimeError(f"{type(self).__name__}.step(): no parameter has a gradient")
        grads = [p.grad.detach().clone() for p in act]
        self._adopt(act)
        with torch.no_grad():
            for p, g in zip(act, grads):
                p.grad.copy_(g)
        self._apply_pending()

    def prebuild(self, params):
        """Fix the flat layout before the first backward (data-parallel runs: a rank may have to join a gradient exchange
        before its own first keyframe).  `params`: the parameters that will receive gradients, in a rank-independent order."""
        if self.flat is not None:
            return
        known = {id(p) for p in self._all}
        act = [p for p in params if p.requires_grad and id(p) in known]
        if not act:
            raise RuntimeError(f"{type(self).__name__}.prebuild(): no trainable parameter")
        self._adopt(act)
        self._apply_pending()

    # ---- torch-compatible state (train_depth.py:849-863 resumes from `<optimizer>.pth`) ---------------------------------------------
    def _has_state(self):
        return self.steps_done() > 0 or self._loaded

    def state_dict(self):
        """The optimiser state in the corresponding torch optimiser's own format -- {"state": {param index: {["step",] STATE keys}},
        "param_groups": [...]} with indices into the parameter list the optimiser was built on -- so a file written here loads into the
        reference's optimiser and vice versa.  Parameters that never received a gradient carry no state, and there is none before the
        first step."""
        groups = []
        start = 0
        for g in self.param_groups:
            d = {k: v for k, v in g.items() if k != "params"}
            d["params"] = list(range(start, start + len(g["params"])))
            start += len(g["params"])
            groups.append(d)
        state = {}
        if self.flat is None and getattr(self, "_pending", None):
            state = {i: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()} for i, st in self._pending.items()}     # loaded, not applied yet
        elif self.flat is not None and self._has_state():                      # like torch: no state before the first step
            t = float(self.steps_done())
            idx = {id(p): i for i, p in enumerate(self._all)}
            for p, o in zip(self.flat.params, self.flat.offsets):
                n = p.numel()
                st = {"step": torch.tensor(t)} if self.STEP_IN_STATE else {}
                st.update({key: getattr(self, attr)[o:o + n].view_as(p).clone() for key, attr in self.STATE})
                state[idx[id(p)]] = st
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, state_dict):
        """Counterpart of torch.optim.Optimizer.load_state_dict for the flat layout: hyper-parameters, state arrays and step count.
        WHICH parameters the flat bucket holds is decided where it always is -- at prebuild() (the caller names the parameters that
        take part) or at the first step() (those with a gradient) -- never by the file: loaded before that, the state waits and is
        applied when the bucket exists.  There is ONE step counter for the bucket, torch keeps one per parameter; they are equal in
        any file a run of the same optimiser over the same parameters wrote.  Where the update depends on the count (Adam), a bucket
        parameter WITHOUT state in a file whose others have stepped (torch would start it at step 0 with its own bias correction)
        cannot be represented and raises instead of being silently mis-stepped or -- round 3 -- silently left out of the bucket and
        never updated.  Where it does not (SGD, RMSprop, Adagrad) such a parameter starts from zero state, which is what
        torch gives it, and the counter takes the largest count in the file."""
        groups = state_dict["param_groups"]
        if len(groups) != 1 or len(self.param_groups) != 1:
            raise NotImplementedError(self._one_group())
        if len(groups[0]["params"]) != len(self._all):
            raise ValueError("loaded state dict has a different number of parameters")
        src = groups[0]
        self._refuse(src)
        self.param_groups[0].update({k: v for k, v in src.items() if k in self.HYPER})
        self._hyper_key = None                              # the hyper-parameters may have changed: rewrite what the device holds at the next step
        state = {int(k): v for k, v in state_dict["state"].items()}
        first = self.STATE[0][0]
        for i, st in state.items():
            if not 0 <= i < len(self._all):
                raise ValueError(f"state for parameter index {i}: the optimiser has {len(self._all)} parameters")
            if st.get(first) is not None and tuple(st[first].shape) != tuple(self._all[i].shape):
                raise ValueError(f"parameter {i}: state of shape {tuple(st[first].shape)} for a parameter of shape {tuple(self._all[i].shape)}")
        self._pending = state or None
        if self.flat is not None:
            self._apply_pending()

    def _apply_pending(self):
        state, self._pending = getattr(self, "_pending", None), None
        if not state:
            return
        idx = {id(p): i for i, p in enumerate(self._all)}
        offs = {idx[id(p)]: (o, p.numel()) for p, o in zip(self.flat.params, self.flat.offsets)}
        steps = {int(float(st["step"])) for st in state.values() if "step" in st}
        if self.STEP_IN_UPDATE:
            if len(steps) != 1:
                raise ValueError(f"per-parameter step counts differ ({sorted(steps)}): the fused optimiser keeps one")
            t = steps.pop()
            missing = sorted(i for i in offs if i not in state)
            if missing and t != 0:
                raise ValueError(f"parameters {missing} are trained here but carry no state in the loaded file, whose other parameters are at "
                                 f"step {t}: torch.optim.Adam would run them on their own step count, the fused optimiser keeps one")
        else:
            t = max(steps, default=0)
            # torch.optim.Adagrad writes zero state for EVERY parameter from its construction on, frozen ones included: state that
            # never moved says nothing about a parameter
            state = {i: st for i, st in state.items() if i in offs or any(torch.is_tensor(st.get(k)) and bool(st[k].any()) for k, _ in self.STATE)}
        extra = sorted(i for i in state if i not in offs and self._all[i].requires_grad)
        if extra:
            raise ValueError(f"parameters {extra} carry optimiser state but are not part of the flat bucket (not among the parameters "
                             "named to prebuild() / without a gradient at the first step)")
        with torch.no_grad():
            for i, st in state.items():
                if i in offs:
                    o, n = offs[i]
                    for key, attr in self.STATE:
                        if st.get(key) is not None:                             # torch.optim.SGD(momentum=0) stores None
                            getattr(self, attr)[o:o + n].copy_(st[key].reshape(-1))
        self._resident_state()
        self._counter.fill_(t + 1)
        self._loaded = True

    def zero_grad(self, set_to_none=True):
        if self.flat is None:
            for p in self._all:
                p.grad = None
        else:
            self.flat.zero_grad()

    @torch.no_grad()
    def step(self, closure=None):
        if self.flat is None:
            self._build()
        self.steps += 1
        self.flat.touched()                            # the kernel rewrites the weights behind torch's version counters
        # the bucket holds the SUM over the data-parallel ranks and its tail the number of contributors (1 on a single GPU); step count
        # and learning rate are device-resident, so this launch can be captured into a hipGraph and replayed
        self.sync_hyperparameters()
        self._launch(self.param_groups[0])


class FusedAdam(FusedOptimizer):
    """torch.optim.Adam(lr, betas=(0.9,0.999), eps=1e-8) semantics (the reference's optimiser:
    utils/training_utils.py:23-25) in one HIP launch."""

    STATE = (("exp_avg", "m"), ("exp_avg_sq", "v"))
    HYPER = ("lr", "betas", "eps")
    STEP_IN_UPDATE = True
    SCHEDULE_LEN = 1 << 18          # bias-correction table: 262 144 steps x 8 B (a 60-frame sequence takes 177)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        # weight_decay / amsgrad: torch.optim.Adam's remaining defaults, carried (at their off values) so that a state dict written here
        # is a complete torch.optim.Adam state dict
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False))
        self._sched = None

    def _refuse(self, group):
        if group.get("weight_decay", 0) or group.get("amsgrad", False) or group.get("maximize", False):
            raise NotImplementedError("FusedAdam: weight_decay / amsgrad / maximize are not on the reference's path (training_utils.py:23-25)")

    def _has_state(self):
        return self.steps_done() > 0

    def _resident_state(self):
        """Device-resident step counter + the per-step scalars {lr / (1 - beta1^t), sqrt(1 - beta2^t)}, computed on the host in
        double exactly as torch.optim.Adam does and rounded to fp32 once; rebuilt in place when lr / betas change."""
        g = self.param_groups[0]
        key = (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]))
        dev = self.flat.data.device
        if self._counter is None:
            self._counter = torch.ones(1, device=dev, dtype=torch.int32)
            self._sched = torch.empty(self.SCHEDULE_LEN, 2, device=dev, dtype=torch.float32)
        if self._hyper_key != key:
            t = torch.arange(1, self.SCHEDULE_LEN + 1, dtype=torch.float64)
            bc1 = 1.0 - torch.pow(torch.tensor(key[1], dtype=torch.float64), t)
            bc2 = 1.0 - torch.pow(torch.tensor(key[2], dtype=torch.float64), t)
            self._sched.copy_(torch.stack([key[0] / bc1, torch.sqrt(bc2)], 1).to(torch.float32))
            self._hyper_key = key
        return self._sched, self._counter

    def _launch(self, g):
        sched, counter = self._resident_state()
        L.call("e2e_adam_step_resident", params=L.ptr(self.flat.data), grad_sums=L.ptr(self.flat.grad), participants=L.ptr(self.flat.participants()),
               exp_avg=L.ptr(self.m), exp_avg_sq=L.ptr(self.v), n=self.flat.numel, beta1=float(g["betas"][0]), beta2=float(g["betas"][1]),
               eps=float(g["eps"]), schedule=L.ptr(sched), schedule_len=self.SCHEDULE_LEN, step_counter=L.ptr(counter), stream=L.stream())


def _refuse_options(name, group, off):
    """`off`: {torch option: its off value}.  The first one `group` sets otherwise is named."""
    for key, value in off.items():
        if group.get(key, value) != value:
            raise NotImplementedError(f"{name}: {key}={group[key]!r} is not implemented by the fused kernel (only {key}={value!r}; "
                                      f"utils/training_utils.py:26-47 never sets it)")


class FusedSGD(FusedOptimizer):
    """torch.optim.SGD(lr, momentum=0.9, weight_decay=1e-3) as the reference builds it (utils/training_utils.py:29-35; dampening 0, no
    nesterov) in one HIP launch: d = g + weight_decay p; buf = momentum buf + d; p -= lr buf.  torch keeps no step count for SGD, so
    a loaded file sets none: steps_done() counts from the load."""

    STATE = (("momentum_buffer", "buf"),)
    HYPER = ("lr", "momentum", "weight_decay")
    STEP_IN_STATE = False

    def __init__(self, params, lr=1e-3, momentum=0.9, weight_decay=1e-3, dampening=0, nesterov=False, maximize=False):
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("FusedSGD: lr, momentum and weight_decay must be >= 0")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=maximize))

    def _refuse(self, group):
        _refuse_options("FusedSGD", group, dict(nesterov=False, dampening=0, maximize=False))

    def _launch(self, g):
        lr, counter = self._resident_state()
        L.call("e2e_sgd_step_resident", params=L.ptr(self.flat.data), grad_sums=L.ptr(self.flat.grad), participants=L.ptr(self.flat.participants()),
               momentum_buffer=L.ptr(self.buf), n=self.flat.numel, lr=L.ptr(lr), momentum=float(g["momentum"]), weight_decay=float(g["weight_decay"]),
               step_counter=L.ptr(counter), stream=L.stream())


class FusedRMSprop(FusedOptimizer):
    """torch.optim.RMSprop(lr, alpha=0.99, eps=1e-8) as the reference builds it (utils/training_utils.py:37-41; no momentum, not
    centred, no weight decay) in one HIP launch: v = alpha v + (1 - alpha) g g; p -= lr g / (sqrt(v) + eps)."""

    STATE = (("square_avg", "v"),)
    HYPER = ("lr", "alpha", "eps")

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False, maximize=False):
        if lr < 0 or not 0 <= alpha <= 1 or eps <= 0:
            raise ValueError("FusedRMSprop: lr >= 0, 0 <= alpha <= 1 and eps > 0 are required")
        super().__init__(params, dict(lr=lr, momentum=momentum, alpha=alpha, eps=eps, centered=centered, weight_decay=weight_decay, maximize=maximize))

    def _refuse(self, group):
        _refuse_options("FusedRMSprop", group, dict(centered=False, momentum=0, weight_decay=0, maximize=False))

    def _launch(self, g):
        lr, counter = self._resident_state()
        L.call("e2e_rmsprop_step_resident", params=L.ptr(self.flat.data), grad_sums=L.ptr(self.flat.grad), participants=L.ptr(self.flat.participants()),
               square_avg=L.ptr(self.v), n=self.flat.numel, lr=L.ptr(lr), alpha=float(g["alpha"]), eps=float(g["eps"]),
               step_counter=L.ptr(counter), stream=L.stream())


class FusedAdagrad(FusedOptimizer):
    """torch.optim.Adagrad(lr, eps=1e-10) as the reference builds it (utils/training_utils.py:43-47; lr_decay 0, accumulator from 0, no
    weight decay) in one HIP launch: s += g g; p -= lr g / (sqrt(s) + eps)."""

    STATE = (("sum", "acc"),)
    HYPER = ("lr", "eps")

    def __init__(self, params, lr=1e-2, lr_decay=0, weight_decay=0, initial_accumulator_value=0, eps=1e-10, maximize=False):
        if lr < 0 or eps <= 0:
            raise ValueError("FusedAdagrad: lr >= 0 and eps > 0 are required")
        super().__init__(params, dict(lr=lr, lr_decay=lr_decay, eps=eps, weight_decay=weight_decay, initial_accumulator_value=initial_accumulator_value,
                                      maximize=maximize))

    def _refuse(self, group):
        _refuse_options("FusedAdagrad", group, dict(lr_decay=0, weight_decay=0, initial_accumulator_value=0, maximize=False))

    def _launch(self, g):
        lr, counter = self._resident_state()
        L.call("e2e_adagrad_step_resident", params=L.ptr(self.flat.data), grad_sums=L.ptr(self.flat.grad), participants=L.ptr(self.flat.participants()),
               sum=L.ptr(self.acc), n=self.flat.numel, lr=L.ptr(lr), eps=float(g["eps"]), step_counter=L.ptr(counter), stream=L.stream())
