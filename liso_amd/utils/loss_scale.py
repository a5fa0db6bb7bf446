"""Loss scaling for fp16 training of the detector, with its state on the device (include/liso_optim.h, liso_loss_scale_state).

fp16 keeps 11 significand bits but only covers 6e-8 .. 65504: the gradients of a loss that is a mean over B x 512 x 512 BEV cells
are ~1e-6 per element and would lose most of their bits (or flush to zero) in fp16 tensors.  The backward pass is therefore seeded
with `scale` instead of 1, and the update divides it out again -- torch.cuda.amp.GradScaler's scheme, except that nothing here syncs
with the host inside a step: the seed is a view of the device state (a captured hipGraph reads the current value on every replay),
the overflow check, the gated AdamW update and the scale update are three launches behind the backward pass (FlatAdamW.step).

Defaults (GradScaler's own are 2^16 / 2000 for arbitrary networks):
  init_scale = 2^9: measured on the MI355X with random-init weights, the first step's fp16 gradients overflowed at a scale of 4096 in two
      of the configurations tried (B = 2 / 256^2, configs[4] at 1024^2), 2048 then ran 34 steps of configs[4] without one; 512 leaves 8x headroom
      below that on the first steps, and the per-element BEV gradients of the mean-reduced losses (~1e-6 at B = 4, 512^2) still land at
      ~5e-4, inside fp16's normal range (>= 6.1e-5);
  growth_interval = 500: training runs here are a few thousand steps per round, so the scale can climb back after a back-off within a
      round (GradScaler's 2000 would take most of it);
  growth_factor 2, backoff_factor 0.5: GradScaler's.
A fixed scale (loss_scale=<float>) is growth = backoff = 1: overflowing steps are still skipped, the scale never moves."""
import torch

from liso_amd import _lib as L

DEFAULT_INIT_SCALE = 2.0 ** 9
DEFAULT_GROWTH_INTERVAL = 500


class DeviceLossScale:
    def __init__(self, device, init_scale=DEFAULT_INIT_SCALE, dynamic=True, growth_interval=DEFAULT_GROWTH_INTERVAL, growth_factor=2.0,
                 backoff_factor=0.5):
        if not init_scale > 0:
            raise ValueError(f"loss scale must be positive, got {init_scale}")
        self.dynamic = bool(dynamic)
        self.growth_interval = int(growth_interval)
        self.growth_factor = float(growth_factor) if dynamic else 1.0
        self.backoff_factor = float(backoff_factor) if dynamic else 1.0
        self.state = torch.zeros(L.LOSS_SCALE_STATE_BYTES // 4, dtype=torch.int32, device=device)
        # the backward seed: a 0-dim fp32 view of `scale` (field 0), read from device memory wherever the backward pass runs
        self.seed = self.state.view(torch.float32)[0]
        self.set_scale(init_scale)

    def set_scale(self, value):
        """host write of the current scale (between steps; tests and checkpoint restore)"""
        self.state.view(torch.float32)[0].fill_(float(value))

    def stats(self):
        """{scale, applied_steps, skipped_steps, growth_tracker} -- reads the device state (a sync; never called inside a step)"""
        s = self.state.cpu()
        return {"scale": float(s.view(torch.float32)[0]), "applied_steps": int(s[3]), "skipped_steps": int(s[4]),
                "growth_tracker": int(s[2])}

    def state_dict(self):
        """what a checkpoint keeps (GradScaler.state_dict's counterpart): the scale, the growth tracker, applied / skipped steps"""
        return dict(self.stats(), growth_interval=self.growth_interval, growth_factor=self.growth_factor,
                    backoff_factor=self.backoff_factor, dynamic=self.dynamic)

    def load_state_dict(self, sd):
        """restores a state_dict() (between steps; the per-step overflow flag starts clear)"""
        self.dynamic = bool(sd.get("dynamic", self.dynamic))
        self.growth_interval = int(sd.get("growth_interval", self.growth_interval))
        self.growth_factor = float(sd.get("growth_factor", self.growth_factor))
        self.backoff_factor = float(sd.get("backoff_factor", self.backoff_factor))
        host = torch.zeros(L.LOSS_SCALE_STATE_BYTES // 4, dtype=torch.int32)
        host.view(torch.float32)[0] = float(sd["scale"])
        host[2], host[3], host[4] = int(sd["growth_tracker"]), int(sd["applied_steps"]), int(sd["skipped_steps"])
        self.state.copy_(host)

    def adamw_step(self, flat_param, flat_grad, flat_exp_avg, flat_exp_avg_sq, numel, lr, beta1, beta2, eps, weight_decay, grad_scale):
        """(a) non-finite check of the gradient buffer, (b) AdamW on grad * grad_scale / scale unless (a) found an inf / NaN, (c) scale
        update -- three launches on the current stream, no host sync"""
        lib, st, sp = L.lib(), L.stream_ptr(), L.ptr(self.state)
        L.check(L.TIMER.launch("grad_nonfinite", lambda: lib.liso_grad_nonfinite_f32(L.ptr(flat_grad), numel, sp, st), units=4 * numel),
                "grad_nonfinite")
        L.check(L.TIMER.launch("adamw_amp", lambda: lib.liso_adamw_step_amp_f32(
            L.ptr(flat_param), L.ptr(flat_grad), L.ptr(flat_exp_avg), L.ptr(flat_exp_avg_sq), numel, float(lr), float(beta1),
            float(beta2), float(eps), float(weight_decay), float(grad_scale), sp, st), units=28 * numel), "adamw_step_amp")
        L.check(lib.liso_loss_scale_update(sp, self.growth_factor, self.backoff_factor, self.growth_interval, st), "loss_scale_update")
