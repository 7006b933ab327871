"""Hook plumbing of the reference's BaseModel (src/models/base.py:4-63).  With pytorch_lightning installed this IS a
LightningModule; without it (this image) a small stand-in offers the attributes the hooks use — `trainer`, `current_epoch`,
`optimizers()`, `manual_backward`, `log_dict`, `save_hyperparameters`, `on_save/on_load_checkpoint` — and
src/tasks/runner.py::Trainer drives them in Lightning 1.6's order."""
import torch
import torch.nn as nn

try:                                            # use Lightning when the environment has it
    from pytorch_lightning import LightningModule as _Base
except Exception:                               # pragma: no cover - not installed in this image
    class _Base(nn.Module):
        automatic_optimization = True
        trainer = None

        def save_hyperparameters(self, *a, **k):
            pass

        def log_dict(self, d, **k):
            self._logged = dict(d)
            if self.trainer is not None:
                self.trainer.callback_metrics.update(d)

        def log(self, name, value, **k):
            self.log_dict({name: value})

        @property
        def device(self):
            return next(self.parameters()).device

        @property
        def current_epoch(self):
            return self.trainer.current_epoch if self.trainer is not None else 0

        def optimizers(self):
            opts = self.trainer.optimizers
            return opts[0] if len(opts) == 1 else opts

        def manual_backward(self, loss, *a, **k):
            loss.backward(*a, **k)

        def on_save_checkpoint(self, checkpoint):
            pass

        def on_load_checkpoint(self, checkpoint):
            pass


class BaseModel(_Base):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.save_hyperparameters(logger=False)

    def training_step(self, batch, batch_idx):
        return self.allsplit_step("train", batch, batch_idx)

    def validation_step(self, batch, batch_idx):
        return self.allsplit_step("val", batch, batch_idx)

    def test_step(self, batch, batch_idx):
        return self.allsplit_step("test", batch, batch_idx)

    def _epoch_dico(self, losses, split):
        """base.py:37-40: the accumulated means under their log names; the accumulator starts over for the next epoch
        (torchmetrics resets a Metric the trainer logs at epoch end; the reference relies on that)."""
        dico = {losses.loss2logname(name, split): float(value) for name, value in losses.compute().items()}
        losses.reset()
        return dico

    def allsplit_epoch_end(self, split, outputs):                         # base.py:36-54
        dico = self._epoch_dico(self.losses[split], split)
        dico.update({"epoch": float(self.trainer.current_epoch), "step": float(self.trainer.current_epoch)})
        if split == "val" and self.current_epoch % 10 == 0:
            self.render_sample_results()
        self.log_dict(dico)

    def training_epoch_end(self, outputs):
        return self.allsplit_epoch_end("train", outputs)

    def validation_epoch_end(self, outputs):
        return self.allsplit_epoch_end("val", outputs)

    def test_epoch_end(self, outputs):
        return self.allsplit_epoch_end("test", outputs)

    # ---- GIF export of sampled clips (gsdd_amd.gif); off unless `render_dir` is set
    render_dir, render_fps, render_max, render_refine, render_dither, render_optimize, render_tolerance = None, 5, 16, 0, 0, False, 0

    def _render_setup(self, render_dir, render_fps, render_max, render_refine=0, render_dither=0, render_optimize=False, render_tolerance=0):
        self.render_dir = str(render_dir) if render_dir not in (None, "", "__None__") else None
        self.render_fps, self.render_max = render_fps, int(render_max)
        # the quantiser's k-means passes (0 .. 32) and dither (an ordered-dither amplitude 0 .. 64, or "fs"): gsdd_amd.gif.quantize_clips
        self.render_refine, self.render_dither = render_refine, render_dither
        # delta frames (transparent pixels where the picture stays, cropped frames) and their tolerance, a squared RGB distance:
        # gsdd_amd.gif.write_gifs(optimize=, tolerance=)
        self.render_optimize, self.render_tolerance = bool(render_optimize), int(render_tolerance)
        self._rendered = 0                                       # clips written by the test split so far

    def _write_gifs(self, clips, directory, names, captions):
        """clips (N, 3, T, H, W) on the device -> <directory>/<name> each, and one `<name>\\t<caption>` line each in captions.txt"""
        import os
        from gsdd_amd.gif import write_gifs
        # with delta frames every group keeps one palette index free for the transparent pixels: 255 colours
        optimize = dict(optimize=True, tolerance=self.render_tolerance, colors=255) if self.render_optimize else {}
        write_gifs(clips.detach().float(), [os.path.join(directory, n) for n in names], fps=self.render_fps,
                   refine=self.render_refine, dither=self.render_dither, **optimize)
        with open(os.path.join(directory, "captions.txt"), "a") as f:
            for n, c in zip(names, captions):
                f.write(f"{n}\t{' '.join(str(c).split())}\n")

    def _long_frames(self):
        """The generator's sample_long_frames when it renders long clips (a DiscreteDiffusion over an autoencoder), else None."""
        n = getattr(getattr(self, "generator", None), "sample_long_frames", None)
        return n if isinstance(n, int) and getattr(self, "autoencoder", None) is not None else None

    def _sample_long_clips(self, batch, limit):
        """The first `limit` items of `batch` as long clips (B, 3, n d_t, H, W): sampled here with the generator's sliding-window
        rollout and decoded with the stitched decode -- the evaluation's one-window sample is neither reused nor touched.  With
        sample_condition_frames the rollout's first window keeps those latent frames of the item's own clip."""
        import contextlib
        gen, auto, n = self.generator, self.autoencoder, self._long_frames()
        texts = list(batch["text"])[:limit]
        was_training = gen.training
        gen.eval()
        try:
            with torch.no_grad(), (self.ema_scope() if hasattr(self, "ema_scope") else contextlib.nullcontext()):
                known_kw = {}
                if gen.sample_condition_frames is not None:
                    quant = auto.encode(batch["video"][:limit].to(auto.device))
                    known_kw = {"known_tokens": quant.view(quant.shape[0], -1),
                                "known_mask": gen.condition_frame_mask(tuple(quant.shape[1:])), "latent_shape": tuple(quant.shape[1:])}
                return gen.sample_videos(texts, auto, long_frames=n, **known_kw)
        finally:
            gen.train(was_training)

    def render_test_batch(self, batch, batch_idx, sampled=None):
        """Test split with `render_dir` set: the batch's sampled clips as <render_dir>/test/<batch_idx>_<i>.gif, at most `render_max`
        in all (`render_dir` alone switches this on: the shipped configs keep `render_animations`, the validation item's switch,
        off).  `sampled`: what do_evaluation has already sampled for this batch (reused); None = the sample is made here.
        With the generator's sample_long_frames set the clips written are long ones, sampled here (`_sample_long_clips`): `sampled` is
        not used, and the extra rollout draws from the sampler's noise stream, so the evaluation samples of LATER batches start at
        another stream offset than in a run without sample_long_frames -- metrics of two such runs are not sample for sample the same."""
        if not self.render_dir or self._rendered >= self.render_max:
            return
        import os
        if self._long_frames() is not None:
            sampled = {"pred_data": self._sample_long_clips(batch, self.render_max - self._rendered)}
        elif sampled is None:
            was_training = self.generator.training
            self.generator.eval()
            with torch.no_grad():
                sampled = self.sample_generator_step(batch)
            self.generator.train(was_training)
        clips = sampled["pred_data"][:self.render_max - self._rendered]
        text = batch.get("text") if isinstance(batch.get("text"), (list, tuple)) else [""] * clips.shape[0]
        names = [f"{batch_idx}_{i}.gif" for i in range(clips.shape[0])]
        self._write_gifs(clips, os.path.join(self.render_dir, "test"), names, text[:clips.shape[0]])
        self._rendered += clips.shape[0]

    def render_sample_results(self):
        """The reference writes animations of one validation item through matplotlib and ffmpeg (multistage_text_motion_model.py:
        254-281).  Here the sampled clips of that item are kept on `self.last_sample`, and with `render_dir` set they are written
        as <render_dir>/epoch_<n>/pred.gif next to the item itself as gt.gif (gsdd_amd.gif: quantiser on the device, GIF89a writer
        in the library).  Rendering runs outside the sampling loop and outside any captured graph; it synchronises."""
        if not getattr(self, "render_animations", False) or self.trainer is None:
            return
        loader = self.trainer.datamodule.val_dataloader()
        batch = next(iter(loader), None)
        if batch is None:
            return
        one = {k: (v[:1] if torch.is_tensor(v) or isinstance(v, list) else v) for k, v in batch.items()}
        was_training = self.generator.training
        self.generator.eval()
        with torch.no_grad():
            self.last_sample = self.sample_generator_step(one)
        self.generator.train(was_training)
        if self.render_dir:
            import os
            pred = self.last_sample["pred_data"] if self._long_frames() is None else self._sample_long_clips(one, 1)      # (pred.gif long)
            caption = one["text"][0] if isinstance(one.get("text"), (list, tuple)) and one["text"] else ""
            directory = os.path.join(self.render_dir, f"epoch_{self.current_epoch}")
            self._write_gifs(pred[:1], directory, ["pred.gif"], [caption])
            self._write_gifs(one["video"][:1].to(pred.device), directory, ["gt.gif"], [caption])

    # ---- state that is not in state_dict but decides the next training step (exact resume)
    def _diffusion_models(self):
        from gsdd_amd.d3pm import DiffusionTransformer
        return [m for m in self.modules() if isinstance(m, DiffusionTransformer)]

    def on_save_checkpoint(self, checkpoint):
        dms = self._diffusion_models()
        checkpoint["gsdd"] = {"noise": [(m.noise_seed, m.noise_stream, m.row_offset) for m in dms],
                              "rng_cpu": torch.get_rng_state(),
                              "rng_cuda": torch.cuda.get_rng_state() if torch.cuda.is_available() else None,
                              "need_init": [bool(getattr(m, "_need_init")) for m in self.modules() if hasattr(m, "_need_init")]}

    def on_load_checkpoint(self, checkpoint):
        st = checkpoint.get("gsdd")
        if not st:
            return
        for m, (seed, stream, row) in zip(self._diffusion_models(), st["noise"]):
            m.set_noise(seed, stream, row)
        torch.set_rng_state(st["rng_cpu"].cpu())
        if st.get("rng_cuda") is not None and torch.cuda.is_available():
            torch.cuda.set_rng_state(st["rng_cuda"].cpu())
        for m, flag in zip([m for m in self.modules() if hasattr(m, "_need_init")], st["need_init"]):
            m._need_init = flag
