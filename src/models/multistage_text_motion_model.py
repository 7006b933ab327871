"""Stage-2 wrapper (D3PM over VQ-VAE tokens): the reference's MultistageTextMotionModel
(src/models/multistage_text_motion_model.py:21-281): same constructor keys, generator_step / sample_generator_step through the
generator glue, manual optimisation (zero_grad -> manual_backward -> step, :186-200), ComputeLosses per model and split,
epoch-end log keys, optimisers (opt_gen, opt_auto) = Adam(betas (0.5, 0.999)).

Deliberate differences, each behind a flag that restores the reference's behaviour:
  * `autoencoder_train_mode=False`: the VQ-VAE stays in eval() whatever `.train()` is called on the wrapper.  The reference never
    freezes it (:104 is commented out), so there Lightning's `.train()` puts it in train mode and every `encode` moves the
    BatchNorm running statistics and runs the codebook's EMA update on the stage-2 data.  True reproduces that.
    (Its optimiser opt_auto is built in both cases, as in the reference, and never changes a weight: the D3PM loss reaches the
    autoencoder only through arg-min indices, so its parameters have no gradient.)
  * `step_in_eval_splits=False`: the reference calls `opt.step()` for every optimiser in the val/test splits too (:199-200),
    re-applying the last training gradients; not reproduced unless asked for.
  * `native_step=False`: True replaces zero_grad/backward/Adam by gsdd_amd.d3pm_train.D3PMTrainer.step (same arithmetic, one
    arena + one Adam launch, data-parallel all-reduce built in).
  * `native_optim` (with native_step only): the native step's optimiser stage -- max_grad_norm, weight_decay, betas, ema_decay,
    skip_nonfinite, warmup_steps (D3PMTrainer); all off by default.  With an average (ema_decay) and `sample_with_ema` every sampling
    call of the wrapper runs on the averaged weights.  `use_ema` (evaluation): the averaged weights of the checkpoint are loaded into
    the generator."""
import contextlib

import torch

from gsdd_amd.hydra_lite import instantiate
from src.models.base import BaseModel
from src.models.text_motion_model import _make_losses


NATIVE_OPTIM_DEFAULTS = {"max_grad_norm": None, "weight_decay": 0.0, "betas": None, "ema_decay": None, "skip_nonfinite": False,
                         "warmup_steps": None}
EMA_KEY = 'checkpoint["gsdd"]["native_adam"]["ema"]'


def check_native_optim(native_optim, native_step):
    """-> the native_optim keys over their defaults; an unknown key, or any key set without native_step, is an error"""
    opt = dict(NATIVE_OPTIM_DEFAULTS)
    given = dict(native_optim or {})
    unknown = sorted(set(given) - set(opt))
    if unknown:
        raise ValueError(f"native_optim: unknown keys {unknown}; the keys are {sorted(opt)}")
    opt.update(given)
    active = sorted(k for k, v in opt.items() if v != NATIVE_OPTIM_DEFAULTS[k])
    if active and not native_step:
        raise ValueError(f"native_optim.{active[0]} is set but native_step is false: the native_optim keys ({', '.join(active)}) "
                         "configure the native HIP training step only -- set native_step=true, or leave them at their defaults "
                         "(the torch optimiser path is not changed by them)")
    return opt


class MultistageTextMotionModel(BaseModel):
    def __init__(self, generator, autoencoder, generator_losses=None, autoencoder_losses=None, length_estimator_losses=None,
                 checkpoint_paths=None, evaluator=None, freeze_models_dict=None, lr_args={}, render_animations=True,
                 do_evaluation=False, devices="cpu", autoencoder_train_mode=False, step_in_eval_splits=False, native_step=False,
                 native_optim=None, sample_with_ema=True, use_ema=False, render_dir=None, render_fps=5, render_max=16, render_refine=0,
                 render_dither=0, render_optimize=False, render_tolerance=0, **kwargs):
        super().__init__()
        self._render_setup(render_dir, render_fps, render_max, render_refine, render_dither, render_optimize, render_tolerance)
        self.gpu_device = devices if devices == "cpu" else "cuda:" + str(devices[0])
        self.generator = instantiate(generator, device=self.gpu_device, _recursive_=False) if isinstance(generator, dict) else generator
        self.autoencoder = instantiate(autoencoder, device=self.gpu_device, _recursive_=False) \
            if isinstance(autoencoder, dict) else autoencoder
        self.length_estimator = None
        self.keys = ["generator", "autoencoder", "length_estimator"]
        self.load_checkpoints(checkpoint_paths)
        self.generator_losses = _make_losses(generator_losses) if generator_losses is not False else None
        self.autoencoder_losses = _make_losses(autoencoder_losses) if autoencoder_losses else None
        self.length_estimator_losses = _make_losses(length_estimator_losses) if length_estimator_losses else None
        self.losses = (self.generator_losses, self.autoencoder_losses, self.length_estimator_losses)
        self.lr_args = dict(lr_args)
        self.render_animations = render_animations
        self.automatic_optimization = False
        self.loss_dict = {}
        self.do_evaluation = do_evaluation
        self.evaluator = instantiate(evaluator, device=self.gpu_device, _recursive_=False) if do_evaluation else None
        self.autoencoder_train_mode = bool(autoencoder_train_mode)
        self.step_in_eval_splits = bool(step_in_eval_splits)
        self.native_step = bool(native_step)
        self.native_optim = check_native_optim(native_optim, self.native_step)
        self.sample_with_ema, self.use_ema = bool(sample_with_ema), bool(use_ema)
        self._native = None
        if not self.autoencoder_train_mode:
            self.autoencoder.eval()

    def train(self, mode=True):
        super().train(mode)
        if not self.autoencoder_train_mode:
            self.autoencoder.eval()
        return self

    def load_checkpoints(self, checkpoint_paths):
        """:69-70 / :113-122: a path, or {autoencoder|generator: path}; '__None__' / None = nothing to load."""
        from gsdd_amd.checkpoint import load_reference_checkpoint
        paths = checkpoint_paths if isinstance(checkpoint_paths, dict) else {"autoencoder": checkpoint_paths}
        for key in ("generator", "autoencoder"):
            path = paths.get(key)
            if path and path != "__None__":
                load_reference_checkpoint(getattr(self, key), path)

    def generator_step(self, batch):                                    # :149-157
        # (the generator's mapping is kept as it is, not copied into a dict: its two decoded by-products are computed only if read --
        # gsdd_amd.d3pm.LazyOutputs; the stage-2 loss reads `losses` alone)
        outputs = self.generator(batch, self.autoencoder, self.length_estimator)
        outputs["length"] = batch["length"]
        return outputs

    def ema_scope(self):
        """The averaged weights for the duration of a sampling call: the native trainer's ema_weights() when it keeps an average and
        `sample_with_ema` is on (and no such scope is open already), else a context that does nothing."""
        nt = self._native
        if nt is None or not self.sample_with_ema or not nt.has_ema or nt._in_ema:
            return contextlib.nullcontext()
        return nt.ema_weights()

    def sample_generator_step(self, batch):                             # :160-168
        with self.ema_scope():
            outputs = self.generator(batch, self.autoencoder, self.length_estimator, do_inference=True)
            outputs["length"] = batch["length"]         # (the deferred by-products are VQ-VAE decodes of tokens: no transformer weight)
        return outputs

    def _native_train_step(self, batch):
        from gsdd_amd.d3pm_train import D3PMTrainer
        if self._native is None:
            o, lr = self.native_optim, self.lr_args.get("gen_lr", 1e-4)
            kw = {"betas": tuple(o["betas"])} if o["betas"] is not None else {}
            if o["warmup_steps"] is not None:
                from gsdd_amd.d3pm_train import linear_warmup
                kw["lr_schedule"] = linear_warmup(lr, o["warmup_steps"])
            self._native = D3PMTrainer(self.generator.diffusion_model, lr=lr, max_grad_norm=o["max_grad_norm"],
                                       weight_decay=o["weight_decay"], ema_decay=o["ema_decay"], skip_nonfinite=o["skip_nonfinite"], **kw)
            self._native.load_optimizer_state(getattr(self, "_native_state", None))
        from gsdd_amd.parallel import broadcast_buffers, set_rank_noise_rows
        with torch.no_grad():
            x = batch["video"].to(self.autoencoder.device)
            tokens = self.autoencoder.encode(x).view(x.shape[0], -1)
            text_emb = self.generator._text(batch["text"], tokens.device)
        # as the glue does on the reference-shaped path: per-rank noise rows, rank 0's importance-sampling statistics everywhere
        set_rank_noise_rows(self.generator.diffusion_model, x.shape[0])
        broadcast_buffers(self.generator.diffusion_model)
        # (condition dropout: the null condition the reference-shaped path hands the denoiser -- None unless train_cond_drop_prob is on)
        loss = self._native.step(tokens, text_emb, null_cond=self.generator.null_condition(tokens.device))[0]
        self.generator_losses["train"].update({"losses": loss})
        self.loss_dict["generator_loss"] = loss
        return self.loss_dict

    def allsplit_step(self, split, batch, batch_idx):                   # :170-206
        if split == "train" and self.native_step:
            return self._native_train_step(batch)
        optimizers = self.optimizers()
        optimizers = list(optimizers) if isinstance(optimizers, (list, tuple)) else [optimizers]
        outputs = self.generator_step(batch)
        eval_outputs = None
        if self.do_evaluation and split != "train" and len(batch["length"]) != 1 and self.current_epoch % 5 == 0:
            eval_outputs = self.sample_generator_step(batch)
            self.evaluator.push_vals(batch, batch_idx, eval_outputs["pred_data"])
        if split == "test":
            self.render_test_batch(batch, batch_idx, eval_outputs)      # (nothing unless render_dir is set)
        # (the reference zips the optimisers into this loop, :189; outside fit() Lightning hands back no optimisers, the zip is
        # empty and its test split accumulates nothing -- here the losses are accumulated in every split)
        for i, (loss, key) in enumerate(zip(self.losses, [k + "_loss" for k in self.keys])):
            if loss:
                self.loss_dict[key] = loss[split].update(outputs)
                if split == "train":
                    optimizers[i].zero_grad()
                    self.manual_backward(self.loss_dict[key], retain_graph=False)
        if split == "train" or self.step_in_eval_splits:
            for opt in optimizers:
                opt.step()
        return self.loss_dict

    def allsplit_epoch_end(self, split, outputs):                       # :208-238
        s = "total/" + split
        total_dico = {s: 0.0}
        for loss in self.losses:
            if loss:
                dico = self._epoch_dico(loss[split], split)
                dico.update({"epoch": float(self.trainer.current_epoch), "step": float(self.trainer.current_epoch)})
                total = total_dico[s] + dico[s]
                total_dico.update(dico)
                total_dico[s] = total
        if self.do_evaluation and split != "train" and self.current_epoch % 5 == 0:
            with self.ema_scope():
                metrics = self.evaluator.evaluate_metrics(self.trainer.datamodule, self.generator)
            total_dico.update({f"Metrics/{m}-{split}": v for m, v in metrics.items()})
            self.evaluator.reset()
        if split == "val" and self.current_epoch % 10 == 0:
            self.render_sample_results()
        self.log_dict(total_dico)

    def on_save_checkpoint(self, checkpoint):
        super().on_save_checkpoint(checkpoint)
        if self._native is not None:
            checkpoint["gsdd"]["native_adam"] = self._native.optimizer_state()

    def on_load_checkpoint(self, checkpoint):
        super().on_load_checkpoint(checkpoint)
        self._native_state = (checkpoint.get("gsdd") or {}).get("native_adam")
        if self._native is not None:
            self._native.load_optimizer_state(self._native_state)
        if self.use_ema:
            self.load_ema_weights(checkpoint)

    def load_ema_weights(self, checkpoint):
        """Evaluation with `use_ema`: the averaged weights the native step keeps in its optimiser state go into the generator's
        transformer (and, when the optimiser carried it, the learned null embedding).  A checkpoint without them is an error."""
        from gsdd_amd._optim import unflatten
        state = (checkpoint.get("gsdd") or {}).get("native_adam") or {}
        if state.get("ema") is None:
            raise KeyError(f"use_ema: the checkpoint holds no averaged weights: {EMA_KEY} is missing (it is written by a run with "
                           "native_step=true and native_optim.ema_decay set)")
        dm = self.generator.diffusion_model
        shapes = [(n, p.shape) for n, p in dm.transformer.named_parameters()]
        n_tr = sum((p.numel() + 3) & ~3 for _, p in dm.transformer.named_parameters())
        if state["ema"].numel() != n_tr:                          # the learned null embedding rides last
            shapes.append(("empty_text_embed", dm.empty_text_embed.shape))
        avg = unflatten(state["ema"], shapes)
        null = avg.pop("empty_text_embed", None)
        with torch.no_grad():
            for n, p in dm.transformer.named_parameters():
                p.copy_(avg[n])
            if null is not None:
                dm.empty_text_embed.copy_(null.double())
        dm.transformer._packed = None

    def configure_optimizers(self):                                     # :240-252
        b1, b2 = 0.5, 0.999
        opt_gen = torch.optim.Adam(self.generator.parameters(), lr=self.lr_args.get("gen_lr", 1e-4), betas=(b1, b2))
        opt_auto = torch.optim.Adam(self.autoencoder.parameters(), lr=self.lr_args.get("auto_lr", 1e-6), betas=(b1, b2))
        return opt_gen, opt_auto
