"""Optimizer adapter: looks like ``getattr(torch.optim, name)([...])`` to the
code around the hot loop (``param_groups`` list of dicts with ``params`` and
``lr``, ``zero_grad()``, ``step()``, printable — reference
``sykepic/train/train.py:131-138``, ``network.py:101-128``) while the update
itself is one fused multi-tensor kernel launch inside ``libsykepic_hip.so``.
"""

from . import lib

# torch.optim's own defaults: the reference constructs `getattr(optim, name)(groups)` with nothing but `lr`
# (sykepic/train/train.py:131-138), so these are the hyper-parameters a reference run uses.
_DEFAULTS = {
    "SGD": dict(momentum=0.0, weight_decay=0.0),
    "Adam": dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
    "AdamW": dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01),
    "RMSprop": dict(alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0),
    "Adagrad": dict(lr_decay=0.0, weight_decay=0.0, initial_accumulator_value=0.0, eps=1e-10),
    "Adamax": dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
    "NAdam": dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, momentum_decay=4e-3),
    "RAdam": dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0),
    "Adadelta": dict(rho=0.9, eps=1e-6, weight_decay=0.0),
    "ASGD": dict(lambd=1e-4, alpha=0.75, t0=1e6, weight_decay=0.0),
    "Rprop": dict(etas=(0.5, 1.2), step_sizes=(1e-6, 50.0)),
}
# hyper-parameters torch's `step()` reads from a loaded group but does not default (`torch.optim.SGD.__setstate__`
# fills in the others): this path fixes them at torch's defaults, `state_dict()` says so
_TORCH_FIXED = {"SGD": dict(dampening=0.0, nesterov=False)}
_KINDS = {"SGD": lib.OPT_SGD, "Adam": lib.OPT_ADAM, "AdamW": lib.OPT_ADAMW, "RMSprop": lib.OPT_RMSPROP,
          "Adagrad": lib.OPT_ADAGRAD, "Adamax": lib.OPT_ADAMAX, "NAdam": lib.OPT_NADAM, "RAdam": lib.OPT_RADAM,
          "Adadelta": lib.OPT_ADADELTA, "ASGD": lib.OPT_ASGD, "Rprop": lib.OPT_RPROP}


class HipOptimizer:
    def __init__(self, net, name, param_groups, **kw):
        if name not in _DEFAULTS:
            raise ValueError(f"optimizer {name!r} has no MI355X kernel (supported: {sorted(_DEFAULTS)}; LBFGS needs a "
                             "closure the reference's loop does not pass, SparseAdam needs sparse gradients)")
        self.net, self.name = net, name
        self.defaults = dict(_DEFAULTS[name])
        self.defaults.update(kw)
        if len(param_groups) > 3:
            raise ValueError("at most 3 param groups (the reference uses exactly 3)")
        self.param_groups = [dict(g) for g in param_groups]
        while len(self.param_groups) < 3:
            self.param_groups.append({"params": [], "lr": 0.0})
        for g in self.param_groups:
            g["params"] = list(g["params"])
        self.grad_scale = 1.0
        self.sync_groups()

    def sync_groups(self):
        """Push the group membership to the library (after LRWarmup edits)."""
        member = {}
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                if p.key in member:
                    raise ValueError("some parameters appear in more than one parameter group")
                member[p.key] = gi
        for p in self.net.parameters():
            self.net.set_param_group(p.key, member.get(p.key, -1))

    def zero_grad(self, set_to_none=True):
        # gradients are overwritten by every forward_backward
        return None

    def step(self):
        d = lib.OptimDesc()
        d.kind = _KINDS[self.name]
        for i in range(3):
            d.lr[i] = float(self.param_groups[i]["lr"])
        b1, b2 = self.defaults.get("betas", (0.9, 0.999))
        d.beta1, d.beta2 = float(b1), float(b2)
        d.eps = float(self.defaults.get("eps", 1e-8))
        d.weight_decay = float(self.defaults.get("weight_decay", 0.0))
        d.momentum = float(self.defaults.get("momentum", 0.0))
        d.grad_scale = float(self.grad_scale)
        d.alpha = float(self.defaults.get("alpha", self.defaults.get("rho", 0.99)))
        d.momentum_decay = float(self.defaults.get("momentum_decay", 4e-3))
        d.lr_decay = float(self.defaults.get("lr_decay", 0.0))
        d.initial_accumulator_value = float(self.defaults.get("initial_accumulator_value", 0.0))
        if self.name == "ASGD":      # lambd travels in lr_decay, the power alpha in alpha (include/sykepic_hip.h)
            d.lr_decay = float(self.defaults["lambd"])
            d.alpha = float(self.defaults["alpha"])
            if float(self.defaults["t0"]) < 1e5:
                raise ValueError("ASGD: the averaged parameters (t0) are not kept on the MI355X path")
        elif self.name == "Rprop":   # etas in beta1 / beta2, step-size bounds in eps / alpha
            d.beta1, d.beta2 = (float(v) for v in self.defaults["etas"])
            d.eps, d.alpha = (float(v) for v in self.defaults["step_sizes"])
        self.net.optim_step(d)

    # ---- torch.optim.Optimizer.state_dict() / load_state_dict() of the class of the same name ----
    def _slots(self):
        """[(torch's state name, which of the library's two moment buffers holds it)] for this optimizer
        (csrc/train_kernels.hip: sgd_multi_kernel, adam_multi_kernel and the table above opt_generic_kernel)."""
        if self.name == "SGD":
            return [("momentum_buffer", 0)] if float(self.defaults.get("momentum", 0.0)) != 0 else []
        if self.name == "RMSprop":
            return [("square_avg", 1)] + ([("momentum_buffer", 0)] if float(self.defaults.get("momentum", 0.0)) > 0 else [])
        return {"Adam": [("exp_avg", 0), ("exp_avg_sq", 1)], "AdamW": [("exp_avg", 0), ("exp_avg_sq", 1)],
                "RAdam": [("exp_avg", 0), ("exp_avg_sq", 1)], "NAdam": [("exp_avg", 0), ("exp_avg_sq", 1)],
                "Adamax": [("exp_avg", 0), ("exp_inf", 1)], "Adagrad": [("sum", 1)],
                "Adadelta": [("square_avg", 0), ("acc_delta", 1)], "Rprop": [("prev", 0), ("step_size", 1)],
                "ASGD": []}[self.name]

    def state_dict(self):
        """The structure ``torch.optim.<name>.state_dict()`` has: ``param_groups`` with running parameter indices and
        the hyper-parameters, ``state`` per index under torch's names (``step`` a float32 scalar tensor, as torch
        stores it).  A parameter that was never stepped has no entry.  torch's float32 ``step`` / ``mu_product`` are
        lossy copies of the library's int64 / double: the exact values travel under ``spk_exact``, a top-level key
        ``torch.optim.Optimizer.load_state_dict`` ignores."""
        import torch
        groups, state, exact, idx = [], {}, {}, 0
        slots = self._slots()
        for g in self.param_groups:
            ids = []
            for p in g["params"]:
                step, mu = self.net.param_counters(p.key)
                if step > 0:
                    exact[idx] = {"step": step, "mu_product": mu}
                    st = {}
                    if self.name != "SGD":
                        st["step"] = torch.tensor(float(step), dtype=torch.float32)
                    if self.name == "NAdam":
                        st["mu_product"] = torch.tensor(mu, dtype=torch.float32)
                    if self.name == "ASGD":   # eta / mu as torch leaves them after `step` steps; ax = the parameter (t0 large)
                        lr, lam = float(g["lr"]), float(self.defaults["lambd"])
                        st["eta"] = torch.as_tensor(lr / ((1 + lam * lr * step) ** float(self.defaults["alpha"])))
                        st["mu"] = torch.as_tensor(1 / max(1, step - float(self.defaults["t0"])))
                        st["ax"] = p.data
                    for tname, slot in slots:
                        st[tname] = self.net._read_optim_state(p.key, slot, p.shape)
                    if st:                    # plain SGD keeps nothing per parameter
                        state[idx] = st
                ids.append(idx)
                idx += 1
            grp = dict(self.defaults)
            grp.update(_TORCH_FIXED.get(self.name, {}))
            grp["lr"] = g["lr"]
            grp["params"] = ids
            groups.append(grp)
        return {"state": state, "param_groups": groups, "spk_exact": exact}

    def load_state_dict(self, state_dict):
        """Accepts `state_dict()` of this class or of the torch optimizer of the same name over the same parameters in
        the same order: positions map saved indices to this optimizer's parameters, as in torch.  Restores the moments,
        the counters (exact ones where the dict carries them), ``lr`` per group and the hyper-parameters."""
        import torch
        saved = state_dict["param_groups"]
        if len(saved) != len(self.param_groups):
            raise ValueError("loaded state dict has a different number of parameter groups")
        if any(len(s["params"]) != len(g["params"]) for s, g in zip(saved, self.param_groups)):
            raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
        state, exact = state_dict.get("state", {}), state_dict.get("spk_exact", {})
        for s, g in zip(saved, self.param_groups):
            g["lr"] = s["lr"]
            for k in self.defaults:      # one set of hyper-parameters serves every group here
                if k in s and s["params"]:
                    self.defaults[k] = s[k]
        slots = self._slots()            # (SGD / RMSprop: depends on the momentum just loaded)
        used = self.net.train_counters()["steps"] > 0   # a fresh model's moments are zero already
        for s, g in zip(saved, self.param_groups):
            for idx, p in zip(s["params"], g["params"]):
                st, ex = state.get(idx, {}), exact.get(idx)
                if ex is not None:
                    step, mu = int(ex["step"]), float(ex["mu_product"])
                else:
                    step = int(round(float(st["step"]))) if "step" in st else (1 if st.get("momentum_buffer") is not None else 0)
                    mu = float(st["mu_product"]) if "mu_product" in st else 1.0
                self.net.set_param_counters(p.key, step, mu)
                for tname, slot in slots:
                    if st.get(tname) is not None:
                        self.net._load_optim_state(p.key, slot, st[tname])
                    elif step == 0:
                        if used:
                            self.net._load_optim_state(p.key, slot, torch.zeros(p.shape))
                    else:
                        raise ValueError(f"loaded state of parameter {idx} ({p.key}) has no {tname!r}")
        self.sync_groups()

    def __repr__(self):
        lines = [f"{self.name} ("]
        for i, g in enumerate(self.param_groups):
            lines.append(f"Parameter Group {i}")
            for k in sorted(self.defaults):
                lines.append(f"    {k}: {self.defaults[k]}")
            lines.append(f"    lr: {g['lr']}")
            lines.append(f"    params: {len(g['params'])} tensors")
        lines.append(")")
        return "\n".join(lines)
