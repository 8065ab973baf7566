"""Autograd bridge: differentiable wrappers around the native forward/backward launch plans."""
import torch as th

from . import _native as nat


class _MaskedMSE(th.autograd.Function):
    """out[b] = mean_{t,c,h,w}((target - pred)^2 * mask[b,t])  (reference gaussian_diffusion.py:787-788,
    nn.py:86-92).  Forward is one HIP reduction; backward is the closed form
    d/dpred = -2 (target - pred) * mask / inner * grad[b]."""

    @staticmethod
    def forward(ctx, target, pred, mask):
        B, T = pred.shape[0], pred.shape[1]
        frame_inner = pred[0, 0].numel()
        target, pred = target.contiguous(), pred.contiguous()
        m = None if mask is None else mask.reshape(B, T).to(th.float32).contiguous()
        out = th.empty(B, device=pred.device, dtype=th.float32)
        nat.masked_mse(target, pred, m, out, B, T, frame_inner)
        ctx.save_for_backward(target, pred, m)
        return out

    @staticmethod
    def backward(ctx, g):
        target, pred, m = ctx.saved_tensors
        B, T = pred.shape[0], pred.shape[1]
        d = th.empty_like(pred)
        nat.check(nat.lib().lfvdm_masked_mse_bwd(nat.ptr(target), nat.ptr(pred), nat.ptr(m), nat.ptr(g.contiguous().float()),
                                                 nat.ptr(d), B, T, pred[0, 0].numel(), nat.stream()), "lfvdm_masked_mse_bwd")
        return None, d, None


def masked_mse(target, pred, mask):
    return _MaskedMSE.apply(target, pred, mask)


class _TrainLoss(th.autograd.Function):
    """The loss head of a timestep-weighted training step in one launch (lfvdm_train_loss): (mse, eval_mse, loss) with
    mse / eval_mse bitwise ``masked_mse`` under ``mask`` / ``eval_mask`` and loss[b] = mse[b] * wtab[t[b]], the weight gathered
    on the device (``t`` changes under a captured graph).  Only ``loss`` is differentiable, with respect to ``pred``:
    d/dpred = -2 (target - pred) * mask / inner * wtab[t[b]] * grad[b] (lfvdm_train_loss_bwd)."""

    @staticmethod
    def forward(ctx, target, pred, mask, eval_mask, t, wtab):
        B, T = pred.shape[0], pred.shape[1]
        target, pred = target.contiguous(), pred.contiguous()
        t = t.to(th.int64).contiguous()
        m, me = (None if k is None else k.reshape(B, T).to(th.float32).contiguous() for k in (mask, eval_mask))
        mse, eval_mse, loss = (th.empty(B, device=pred.device, dtype=th.float32) for _ in range(3))
        nat.train_loss(target, pred, m, me, t, wtab, mse, eval_mse, loss)
        ctx.save_for_backward(target, pred, m, t, wtab)
        ctx.mark_non_differentiable(mse, eval_mse)
        return mse, eval_mse, loss

    @staticmethod
    def backward(ctx, _g_mse, _g_eval, g):
        target, pred, m, t, wtab = ctx.saved_tensors
        d = th.empty_like(pred)
        nat.train_loss_bwd(target, pred, m, t, wtab, g.contiguous().float(), d)
        return None, d, None, None, None, None


def train_loss(target, pred, mask, eval_mask, t, wtab):
    return _TrainLoss.apply(target, pred, mask, eval_mask, t, wtab)


class _VbTerm(th.autograd.Function):
    """vb[b] of ``GaussianDiffusion._vb_terms_bpd`` with clip_denoised=False (reference gaussian_diffusion.py:687-720, the
    KL training loss): one HIP launch forward (lfvdm_vb_terms), one backward (lfvdm_vb_terms_bwd, the closed-form gradient);
    the gradient goes to the network output only.  ``tabs``: the device tables (recip, recipm1, c1, c2, post_logvar,
    model_logvar), ``mean_type``: _native.MEAN_EPS / MEAN_X0."""

    @staticmethod
    def forward(ctx, x_start, x_t, out, t, mask, tabs, mean_type):
        B, T = out.shape[0], out.shape[1]
        x_start, x_t, out = x_start.contiguous(), x_t.contiguous(), out.contiguous()
        t = t.to(th.int64).contiguous()
        m = None if mask is None else mask.reshape(B, T).to(th.float32).contiguous()
        recip, recipm1, c1, c2, post_lv, model_lv = tabs
        vb = th.empty(B, device=out.device, dtype=th.float32)
        nat.vb_terms(x_start, x_t, out, None, t, recip, recipm1, c1, c2, post_lv, model_lv, m, mean_type, False, vb)
        ctx.save_for_backward(x_start, x_t, out, t, m)
        ctx.tabs, ctx.mean_type = tabs, mean_type
        return vb

    @staticmethod
    def backward(ctx, g):
        x_start, x_t, out, t, m = ctx.saved_tensors
        recip, recipm1, c1, c2, _, model_lv = ctx.tabs
        d = th.empty_like(out)
        nat.vb_terms_bwd(x_start, x_t, out, t, recip, recipm1, c1, c2, model_lv, m, g.contiguous().float(), ctx.mean_type, False, d)
        return None, None, d, None, None, None, None


def vb_term(x_start, x_t, out, t, mask, tabs, mean_type):
    return _VbTerm.apply(x_start, x_t, out, t, mask, tabs, mean_type)


def unet_apply(engine, x, x0, timesteps, frame_indices, obs_mask, latent_mask, return_attn_weights):
    from ._backward import UNetFunction
    return UNetFunction.run(engine, x, x0, timesteps, frame_indices, obs_mask, latent_mask, return_attn_weights)
