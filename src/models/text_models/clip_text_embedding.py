"""Text-conditioning provider with the reference's call contract (src/models/text_models/clip_text_embedding.py:11-69):
`CLIPTextEmbedding(clip_dim=512)(list[str]) -> (B, clip_dim)` float tensor; with `per_token=True` (needs a tower) the token features of
the recipe's 22 context positions instead, (B, 22, clip_dim): the final LayerNorm of every position, no pooling and no projection, the
condition upstream VQ-Diffusion's cross-attention is written for (the training step and the sampler take any number of tokens).

The reference builds a frozen OpenAI CLIP ViT-B/32 text tower through the `clip` package, which downloads its weights (:22-29).
Neither the package nor the weights nor the BPE vocabulary exist offline, and the generator zeroes the embedding anyway
(src/models/networks/discrete_diffusion.py:25, :49), so by default this provider is a deterministic hash embedding that keeps the
contract.  When a LOCAL copy of the text tower is supplied (`weights=<directory>` in the Hugging Face layout: config.json,
model.safetensors, vocab.json, merges.txt of `openai/clip-vit-base-patch32`), the real tower runs instead, reproducing the reference's
recipe: tokenise with context length 22 (start + 20 + end, truncated), zero-pad the ids to 77, take the projected feature at the end-of-text
token (`clip_model.encode_text`, :56-64).  Nothing is ever fetched: the directory must exist.

Where the tower runs: the Hugging Face module `self.clip_model` owns the weights.  On a CPU module it also computes (plain PyTorch, the
path tests/test_host_logic.py checks).  On a GPU module the forward pass is `gsdd_amd.text.ClipTextTower`: the HIP kernels of libgsdd.so,
fp32 (the reference runs the tower in fp16, `clip.model.convert_weights`), built lazily from `clip_model.state_dict()` and rebuilt
after the module moves.  `native=None` (auto: native on a GPU, PyTorch on the CPU) | True (native; an error on a CPU module) | False
(PyTorch wherever the module lives).  **Parity**: the native tower is pinned against the `transformers` implementation on a small
seeded tower (tests/golden/clip_text_small.npz, tests/test_gpu_text_tower.py); it is NOT pinned against ViT-B/32 or against
`clip.encode_text` itself, neither of which exists offline."""
import hashlib
import os

import torch
import torch.nn as nn

from gsdd_amd import GsddError
from gsdd_amd.text import ClipTextTower


class CLIPTextEmbedding(nn.Module):
    MAX_TEXT_LEN = 20                  # :57 (the reference hard-codes HumanML's limit)
    CONTEXT_DEFAULT = 77               # :58

    def __init__(self, clip_dim=512, weights=None, native=None, per_token=False, **kwargs):
        super().__init__()
        self.clip_dim = clip_dim
        self.per_token = bool(per_token)
        self.native = native
        self._tower = None                                         # ClipTextTower of the current device (not a sub-module)
        self.register_buffer("_anchor", torch.zeros(1))
        self.tokenizer, self.clip_model = None, None
        if weights:
            if not os.path.isdir(weights):
                raise FileNotFoundError(f"CLIPTextEmbedding(weights={weights!r}): not a directory; a local copy of the CLIP text tower "
                                        "(config.json, model.safetensors, vocab.json, merges.txt) is needed -- nothing is downloaded")
            from transformers import CLIPTextModelWithProjection, CLIPTokenizer
            self.tokenizer = CLIPTokenizer.from_pretrained(weights, local_files_only=True)
            self.clip_model = CLIPTextModelWithProjection.from_pretrained(weights, local_files_only=True).eval()
            for p in self.clip_model.parameters():                 # load_and_freeze_clip (:27-38)
                p.requires_grad = False
            if self.clip_model.config.projection_dim != clip_dim:
                raise ValueError(f"the supplied tower projects to {self.clip_model.config.projection_dim} dimensions, clip_dim is {clip_dim}")
            if self.per_token and self.clip_model.config.hidden_size != clip_dim:
                raise ValueError(f"per_token=True returns the tower's token features, {self.clip_model.config.hidden_size} wide; "
                                 f"clip_dim is {clip_dim}")

    def train(self, mode=True):                                    # the tower stays frozen in eval mode, as in the reference
        super().train(mode)
        if self.clip_model is not None:
            self.clip_model.eval()
        return self

    def tokenize(self, texts):
        """clip.tokenize(raw_text, context_length=22, truncate=True) + zero padding to 77 (:59-62) -> int64 (B, 77)."""
        ctx = self.MAX_TEXT_LEN + 2
        tk = self.tokenizer
        rows = []
        for t in texts:
            ids = tk(t, add_special_tokens=False)["input_ids"][:ctx - 2]
            ids = [tk.bos_token_id] + ids + [tk.eos_token_id]
            rows.append(ids + [0] * (self.CONTEXT_DEFAULT - len(ids)))
        return torch.tensor(rows, dtype=torch.int64)

    def _native_tower(self, dev):
        if self._tower is None or self._tower.device != dev:
            cfg = self.clip_model.config
            if cfg.hidden_act != "quick_gelu":
                raise GsddError(f"the native text tower implements CLIP's QuickGELU, the supplied tower uses {cfg.hidden_act!r}: "
                                "pass native=False to run it as PyTorch")
            self._tower = ClipTextTower.from_hf_state_dict(self.clip_model.state_dict(), cfg.num_attention_heads,
                                                           eps=cfg.layer_norm_eps).to(dev)
        return self._tower

    @torch.no_grad()
    def forward(self, texts, force_mask=False, native=None, return_lengths=False):
        """return_lengths=True -> (features, lengths): int32 (B,) on the host, a caption's end-of-text position + 1 with per_token (the
        positions that are its own tokens; taken from the ids tokenized here, no device synchronisation), all ones without."""
        out = self._embed(texts, native)
        if not return_lengths:
            return out
        if not self.per_token:
            return out, torch.ones((len(texts),), dtype=torch.int32)
        ids = self.tokenize(texts)
        return out, ((ids == self.tokenizer.eos_token_id).int().argmax(dim=1) + 1).to(torch.int32)

    def _embed(self, texts, native=None):
        dev = self._anchor.device
        native = self.native if native is None else native
        if self.clip_model is None:
            if self.per_token:
                raise GsddError("CLIPTextEmbedding(per_token=True) needs a text tower (weights=<directory>): the hash embedding has no tokens")
            rows = []
            for t in texts:
                seed = int.from_bytes(hashlib.sha256(t.encode()).digest()[:8], "little")
                g = torch.Generator().manual_seed(seed)
                v = torch.randn(self.clip_dim, generator=g)
                rows.append(v / v.norm())
            return torch.stack(rows).to(dev)
        if native and dev.type != "cuda":
            raise GsddError("CLIPTextEmbedding(native=True): the native text tower needs the module on a GPU device (no CPU fallback)")
        if native or (native is None and dev.type == "cuda"):
            ids = self.tokenize(texts)                             # host ids: the end-of-text positions cost no device sync
            eot = (ids == self.tokenizer.eos_token_id).int().argmax(dim=1)
            if self.per_token:
                # the token features of the recipe's fixed context (start + 20 + end = 22 positions, untrimmed: Te is one constant and
                # the captured training step is not re-captured per batch); positions behind a caption's end-of-text are kept, as upstream
                # VQ-Diffusion keeps them -- forward(return_lengths=True) tells the caller where they start, and the denoiser's
                # cross-attention skips them when given those lengths
                ctx = self.MAX_TEXT_LEN + 2
                return self._native_tower(dev)(ids[:, :ctx].contiguous(), eot=eot, trim=False, tokens=True)
            return self._native_tower(dev)(ids, eot=eot)
        ids = self.tokenize(texts).to(dev)
        # encode_text: token + positional embedding, causal transformer, ln_final, the feature AT THE END-OF-TEXT TOKEN times the text
        # projection.  (The zero padding behind it is invisible to that position under the causal mask.)
        hidden = self.clip_model.text_model(input_ids=ids, attention_mask=None).last_hidden_state
        if self.per_token:
            return hidden[:, :self.MAX_TEXT_LEN + 2].float()
        eot = (ids == self.tokenizer.eos_token_id).int().argmax(dim=1)
        pooled = hidden[torch.arange(ids.shape[0], device=dev), eot]
        return self.clip_model.text_projection(pooled).float()
