"""Autograd-path trainer for every model that is not VGG (ResNet family now; the
decoder LM of ``models.llama``): PyTorch-ROCm modules for the layer math, the
framework's own data-parallel runtime around them.

* DDP = ``parallel.ddp.DistributedDataParallel`` (flat gradient buffer, grads as
  bucket views, post-accumulate hooks launch bucketed all-reduce(AVG) while
  autograd is still producing earlier layers' gradients) over the native
  ``RcclComm`` (``comm="rccl"``) or ProcessGroupNCCL (``comm="torch"``);
  or any explicit strategy of ``parallel.sync`` (part2a / part2a_extra / part2b);
* optimizer = ``ops.optim.FusedSGD`` (one multi-tensor HIP launch per step), or with
  ``optimizer="adamw"`` / ``CS744_OPTIMIZER=adamw`` ``ops.optim.FusedAdamW`` (AdamW + global-norm
  gradient clipping: one norm launch, one update launch per parameter group);
* ResNets run the framework's channels-last path by default (``models.resnet`` ``layout="nhwc"``:
  hipBLASLt GEMM convolutions over gfx950 im2col / BatchNorm / pool kernels, no MIOpen);
  ``CS744_RESNET_LAYOUT=nchw`` selects MIOpen convolutions on NCHW with the fused NCHW
  BatchNorm kernels. MIOpen's own channels_last kernels (``CS744_CHANNELS_LAST=1`` with the
  NCHW layout) measured 10-18x SLOWER on MI355X (torch 2.10+rocm7.0: composable_kernel
  weight-gradient kernels up to 225 ms each). Optionally under bf16 autocast
  (``dtype="bf16"``; master weights and the optimizer stay fp32);
* data = device-resident synthetic batches of the named shape (no host traffic); for the LM,
  ``doc_len=N`` / ``CS744_DOC_LEN=N`` packs documents of about N tokens into every row and trains
  with document-masked attention (``ops.attention``), the mask derived from the EOS tokens each step;
  ``loss_mask="doc"`` / ``CS744_LOSS_MASK=doc`` then drops the targets that cross a document boundary
  from the loss, ``z_loss=z`` / ``CS744_Z_LOSS=z`` adds the z-loss (``ops.lm.cross_entropy``), and
  ``evaluate()`` reports the z-free, token-weighted negative log-likelihood and perplexity.
"""
from __future__ import annotations

from typing import Optional

import math
import os

import torch
import torch.nn as nn

from ..parallel import DistributedDataParallel, make_comm, make_sync
from ..utils.metrics import roctx_range


def build_model(name: str, qk_norm: bool = False) -> nn.Module:
    from ..models import resnet, vgg
    n = name.lower().replace("-", "")
    if qk_norm and not (n.startswith("llama") or n.startswith("decoder")):
        raise ValueError(f"qk_norm (the per-head RMSNorm of q and k) is for the LM models, not {name!r}")
    if n.startswith("vgg"):
        return vgg.VGG(n.upper())
    if n in ("resnet18", "resnet34", "resnet50", "resnet101"):
        return getattr(resnet, n)(layout=os.environ.get("CS744_RESNET_LAYOUT", "nhwc"))
    if n.startswith("llama") or n.startswith("decoder"):
        from ..models import llama
        return llama.build(name.lower(), qk_norm=qk_norm)
    raise ValueError(f"unknown model {name!r}")


class SyntheticBatches:
    """A pool of random, fixed, device-resident samples; each step gathers a random batch.

    Images: uint8 NHWC pool -> fp32/bf16 normalised NCHW(channels_last) batch.
    Tokens: int64 [pool, seq+1] -> (input, target) shifted pair. With ``doc_len=N`` every pool row is
    cut into documents once, here: lengths uniform on [max(1, N // 2), 3 N // 2] from the seeded CPU
    generator (drawn after the tokens, which stay those of the undivided pool), the last document
    truncated at the row end, ``eos_id`` written at each document's last position.
    """

    def __init__(self, kind: str, batch: int, device, shape=(3, 224, 224), classes: int = 1000, pool: int = 512,
                 seq: int = 0, vocab: int = 0, seed: int = 0, channels_last: bool = True,
                 doc_len: Optional[int] = None, eos_id: Optional[int] = None):
        self.fmt = torch.channels_last if channels_last else torch.contiguous_format
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.kind, self.batch, self.device = kind, batch, device
        self.pool = max(pool, batch)
        if kind == "image":
            c, h, w = shape
            self.data = torch.randint(0, 256, (self.pool, h, w, c), generator=g, dtype=torch.uint8).to(device)
            self.labels = torch.randint(0, classes, (self.pool,), generator=g).to(device)
            self.mean = torch.tensor([0.485, 0.456, 0.406], device=device).view(1, 3, 1, 1) * 255
            self.std = torch.tensor([0.229, 0.224, 0.225], device=device).view(1, 3, 1, 1) * 255
        else:
            tokens = torch.randint(0, vocab, (self.pool, seq + 1), generator=g)
            if doc_len is not None:
                if doc_len < 1 or eos_id is None or not 0 <= eos_id < vocab:
                    raise ValueError("doc_len needs doc_len >= 1 and an eos_id inside the vocabulary")
                lo, hi, L = max(1, doc_len // 2), 3 * doc_len // 2, seq + 1
                n = L // lo + 1  # documents that certainly cover a row; the one crossing its end is truncated
                ends = torch.randint(lo, hi + 1, (self.pool, n), generator=g).cumsum(1) - 1  # last positions
                eos = torch.zeros(self.pool, L, dtype=torch.bool).scatter_(1, ends.clamp_(max=L - 1), True)
                tokens = tokens.masked_fill(eos, eos_id)
            self.tokens = tokens.to(device)
        self.gen = torch.Generator(device=device).manual_seed(seed + 1)

    def next(self):
        idx = torch.randint(0, self.pool, (self.batch,), device=self.device, generator=self.gen)
        if self.kind == "image":
            x = self.data.index_select(0, idx).permute(0, 3, 1, 2).float()
            x = ((x - self.mean) / self.std).contiguous(memory_format=self.fmt)
            return x, self.labels.index_select(0, idx)
        t = self.tokens.index_select(0, idx)
        return t[:, :-1].contiguous(), t[:, 1:].contiguous()


class TorchTrainer:
    def __init__(self, model: str, batch_size: int, device, rank: int = 0, world: int = 1, sync: str = "ddp",
                 comm: str = "rccl", bucket_mb: float = 25.0, bucket_policy: str = "layer", dtype: str = "fp32",
                 lr: float = 0.1, momentum: float = 0.9, weight_decay: float = 1e-4, seed: int = 5000,
                 seq_len: int = 0, fused_sgd: bool = True, optimizer: Optional[str] = None, betas=(0.9, 0.95),
                 eps: float = 1e-8, max_grad_norm: Optional[float] = None, doc_len: Optional[int] = None,
                 loss_mask: Optional[str] = None, z_loss: Optional[float] = None, fused_head: Optional[bool] = None,
                 fused_residual: Optional[bool] = None, qk_norm: Optional[bool] = None):
        """``doc_len``: pack documents of about that many tokens into every row of the synthetic token
        pool (``SyntheticBatches``) and train with document-masked attention: ``step()`` derives the
        document of every token from the EOS tokens of its input, the way real packed data would be
        handled. ``None`` takes ``CS744_DOC_LEN`` if set, else no document masking. LM models only.

        ``loss_mask="doc"`` (needs ``doc_len``): the target at every EOS input, the first token of the next
        document, which the document mask has made unpredictable, is set to the ignore index -100
        (``ops.lm.mask_boundary_targets``) and takes no loss and no gradient. ``z_loss``: the coefficient
        of the auxiliary ``z * lse^2`` per token. ``None`` takes ``CS744_LOSS_MASK`` / ``CS744_Z_LOSS`` if
        set, else no mask / no z-loss. LM models only. The loss is the mean over the rank's own valid
        tokens; with several ranks the gradient all-reduce then averages the ranks with equal weight
        (the usual convention; not a global valid-token mean). ``tokens_per_step()`` still counts every
        token processed.

        ``fused_head``: run the output projection and the loss together over row chunks
        (``ops.lm.linear_cross_entropy``), so that the [tokens, vocab] logits and their gradient are never
        built whole; ``step()`` hands targets, ignore index and z-loss to the model and ``evaluate()``
        uses ``ops.lm.linear_cross_entropy_sums``. ``None`` takes ``CS744_FUSED_HEAD=1`` if set, else off.
        LM models only. ``CS_LM_HEAD_CHUNK_MB`` sets the chunk size.

        ``fused_residual``: fuse every residual add of the decoder blocks into the RMSNorm that follows
        it (``ops.lm.add_rms_norm``; sets ``Llama.fused_residual``): same parameters, same results, less
        traffic on the residual stream. ``None`` takes ``CS744_FUSED_RESIDUAL=1`` if set, else off. LM
        models only.

        ``qk_norm``: build the decoder with QK-norm (``LlamaConfig.qk_norm``): a per-head RMSNorm of q and
        k with a learned [head_dim] gain each, fused with RoPE (``ops.lm.qk_norm_rope``). It adds the
        parameters ``attention.q_norm.weight`` / ``k_norm.weight`` to every layer (1-D: no weight decay
        under AdamW). ``None`` takes ``CS744_QK_NORM=1`` if set, else off. LM models only.

        ``optimizer``: ``"sgd"`` (momentum SGD, the default) or ``"adamw"`` (AdamW with decoupled weight
        decay on the parameters with ``dim() >= 2`` only, and global-norm gradient clipping at
        ``max_grad_norm`` when that is set). ``None`` takes ``CS744_OPTIMIZER`` if set, else ``"sgd"``;
        only when that variable is set do ``CS744_LR``, ``CS744_WEIGHT_DECAY`` and
        ``CS744_MAX_GRAD_NORM`` replace ``lr``, ``weight_decay`` and ``max_grad_norm``. ``lr`` and
        ``weight_decay`` are used as passed for either optimizer: their defaults (0.1, 1e-4) are SGD's
        and no AdamW setting (a decoder LM wants about ``lr=3e-4, weight_decay=0.1``). ``fused_sgd``
        means "use the fused optimizer" for both (``FusedSGD`` / ``FusedAdamW`` on a GPU)."""
        torch.manual_seed(seed)
        # MIOpen find mode for the CNN convolutions (CS744_CONV_BENCHMARK=1): time every solver
        # once per shape instead of taking the heuristic pick (opt-in: for ResNet-50 the search ran
        # for more than 3 minutes on MI355X before the first step finished)
        if os.environ.get("CS744_CONV_BENCHMARK", "0") == "1":
            torch.backends.cudnn.benchmark = True
        self.device, self.world, self.B = device, world, batch_size
        self.model_name = model
        if qk_norm is None:
            qk_norm = os.environ.get("CS744_QK_NORM", "0") == "1"
        self.qk_norm = bool(qk_norm)
        self.module = build_model(model, qk_norm=self.qk_norm).to(device)
        self.is_lm = hasattr(self.module, "vocab_size")
        self.channels_last = not self.is_lm and os.environ.get("CS744_CHANNELS_LAST", "0") == "1"
        if self.channels_last:
            self.module = self.module.to(memory_format=torch.channels_last)
        self.dtype = dtype
        self.grad_comm_dtype = "fp32"
        if world > 1 and sync == "ddp":
            # gradients travel in fp32 like the reference's DDP; CS744_GRAD_COMM_DTYPE=bf16 halves the
            # all-reduce bytes for the decoder LMs (opt-in: RCCL then sums in bf16 over N ranks, a
            # rounding per hop that no reference fixture pins)
            gdt = os.environ.get("CS744_GRAD_COMM_DTYPE", "fp32")
            self.grad_comm_dtype = gdt
            self.net = DistributedDataParallel(self.module, comm=make_comm(comm), bucket_cap_mb=bucket_mb,
                                               bucket_policy=bucket_policy,
                                               grad_comm_dtype=torch.bfloat16 if gdt == "bf16" else None)
            self.sync = make_sync("none", [])
        else:
            self.net = self.module
            self.sync = make_sync(sync if world > 1 else "none", self.module.parameters())
        if optimizer is None and "CS744_OPTIMIZER" in os.environ:
            optimizer = os.environ["CS744_OPTIMIZER"].lower()
            lr = float(os.environ.get("CS744_LR", lr))
            weight_decay = float(os.environ.get("CS744_WEIGHT_DECAY", weight_decay))
            if "CS744_MAX_GRAD_NORM" in os.environ:
                max_grad_norm = float(os.environ["CS744_MAX_GRAD_NORM"])
        optimizer = "sgd" if optimizer is None else optimizer
        if optimizer not in ("sgd", "adamw"):
            raise ValueError(f"unknown optimizer {optimizer!r} (sgd or adamw)")
        self.optimizer = optimizer
        fused = fused_sgd and torch.cuda.is_available()
        # clipping done here with clip_grad_norm_ (FusedAdamW clips inside its own pass instead)
        self.clip_norm = max_grad_norm
        if optimizer == "adamw":
            from ..ops.optim import FusedAdamW
            named = list(self.net.parameters())
            groups = [{"params": [p for p in named if p.dim() >= 2], "weight_decay": weight_decay},
                      {"params": [p for p in named if p.dim() < 2], "weight_decay": 0.0}]
            groups = [g for g in groups if g["params"]]
            if fused:
                self.opt = FusedAdamW(groups, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      max_grad_norm=max_grad_norm)
                self.clip_norm = None
            else:
                self.opt = torch.optim.AdamW(groups, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        else:
            from ..ops.optim import FusedSGD
            params = self.net.parameters()
            self.opt = FusedSGD(params, lr=lr, momentum=momentum, weight_decay=weight_decay) if fused else \
                torch.optim.SGD(params, lr=lr, momentum=momentum, weight_decay=weight_decay)
        self.crit = nn.CrossEntropyLoss()
        if doc_len is None and "CS744_DOC_LEN" in os.environ:
            doc_len = int(os.environ["CS744_DOC_LEN"])
        if doc_len is not None and not self.is_lm:
            raise ValueError(f"doc_len (document-masked attention) is for the LM models, not {model!r}")
        self.doc_len = doc_len
        if loss_mask is None and "CS744_LOSS_MASK" in os.environ:
            loss_mask = os.environ["CS744_LOSS_MASK"].lower()
        if z_loss is None and "CS744_Z_LOSS" in os.environ:
            z_loss = float(os.environ["CS744_Z_LOSS"])
        if (loss_mask is not None or z_loss is not None) and not self.is_lm:
            raise ValueError(f"loss_mask / z_loss are for the LM models, not {model!r}")
        if loss_mask not in (None, "doc"):
            raise ValueError(f"unknown loss_mask {loss_mask!r} ('doc' or None)")
        if loss_mask == "doc" and doc_len is None:
            raise ValueError("loss_mask='doc' needs doc_len (the documents whose boundaries it masks)")
        if z_loss is not None and not (0.0 <= z_loss < math.inf):
            raise ValueError(f"z_loss must be finite and >= 0, got {z_loss}")
        self.loss_mask, self.z_loss = loss_mask, 0.0 if z_loss is None else float(z_loss)
        if fused_head is None:
            fused_head = os.environ.get("CS744_FUSED_HEAD", "0") == "1"
        if fused_head and not self.is_lm:
            raise ValueError(f"fused_head (the chunked linear + cross-entropy head) is for the LM models, not {model!r}")
        self.fused_head = bool(fused_head)
        if fused_residual is None:
            fused_residual = os.environ.get("CS744_FUSED_RESIDUAL", "0") == "1"
        if fused_residual and not self.is_lm:
            raise ValueError(f"fused_residual (the residual add fused into the RMSNorm) is for the LM models, "
                             f"not {model!r}")
        self.fused_residual = bool(fused_residual)
        if self.is_lm:
            self.module.fused_residual = self.fused_residual
        if self.is_lm:
            self.eos_id = self.module.cfg.eos_id
            self.data = SyntheticBatches("tokens", batch_size, device, seq=seq_len or self.module.max_seq,
                                         vocab=self.module.vocab_size, seed=seed, doc_len=doc_len,
                                         eos_id=self.eos_id if doc_len is not None else None)
        else:
            shape = (3, 32, 32) if model.lower().startswith("vgg") else (3, 224, 224)
            classes = 10 if model.lower().startswith("vgg") else 1000
            # the NHWC ResNet reads the batch channels-last (its permute to [B, H, W, C] is then free)
            nhwc = getattr(self.module, "layout", "nchw") == "nhwc"
            self.data = SyntheticBatches("image", batch_size, device, shape=shape, classes=classes, seed=seed,
                                         channels_last=self.channels_last or nhwc)
        self.loss: Optional[torch.Tensor] = None

    def step(self) -> None:
        x, y = self.data.next()
        self.opt.zero_grad()  # DDP re-attaches its bucket views (and zeroes them) in forward
        with roctx_range("cs.forward"), torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.dtype == "bf16"):
            doc_ids = None
            if self.doc_len is not None:  # packed rows: documents end at the EOS tokens of the input
                from ..ops.attention import doc_ids_from_eos
                doc_ids = doc_ids_from_eos(x, self.eos_id)
            if self.fused_head:  # the model ends in the chunked head + loss: no [tokens, vocab] logits
                loss = self.net(x, doc_ids=doc_ids, targets=self._targets(x, y), ignore_index=self._ignore_index(),
                                z_loss=self.z_loss)
            else:
                out = self.net(x, doc_ids=doc_ids) if doc_ids is not None else self.net(x)
                if self.is_lm:  # fused gfx950 softmax cross-entropy over the bf16 logits (ops.lm)
                    from ..ops.lm import cross_entropy
                    loss = cross_entropy(out.view(-1, out.shape[-1]), self._targets(x, y).view(-1),
                                         ignore_index=self._ignore_index(), z_loss=self.z_loss)
                else:
                    loss = self.crit(out.float(), y)
        with roctx_range("cs.backward"):  # DDP's bucket all-reduces are enqueued from its hooks in here
            loss.backward()
        with roctx_range("cs.sync"):
            self.sync()
        with roctx_range("cs.sgd"):
            if self.clip_norm is not None:
                torch.nn.utils.clip_grad_norm_([p for g in self.opt.param_groups for p in g["params"]],
                                               self.clip_norm)
            self.opt.step()
        self.loss = loss.detach()

    def _ignore_index(self) -> Optional[int]:
        return -100 if self.loss_mask == "doc" else None

    def _targets(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        if self.loss_mask == "doc":
            from ..ops.lm import mask_boundary_targets
            return mask_boundary_targets(x, y, self.eos_id, -100)
        return y

    def evaluate(self, batches: int) -> dict:
        """Forward only over ``batches`` fresh batches of the same pool, in eval mode under ``no_grad``,
        with the trainer's document mask and loss mask: ``{"nll", "ppl", "tokens"}``, the negative
        log-likelihood summed over the valid tokens of all batches divided by their number, its
        exponential, and that number. No z-loss in it: this is the token-weighted figure that the
        training loss no longer is once ``z_loss > 0``. The sums stay on the device and are read back
        once. With several ranks every rank reports its own batches' numbers. LM models only."""
        if not self.is_lm:
            raise ValueError("evaluate() is for the LM models")
        from ..ops.lm import cross_entropy_sums, linear_cross_entropy_sums
        was_training = self.net.training
        self.net.eval()
        acc = torch.zeros(2, dtype=torch.float64, device=self.device)  # (nll sum, valid tokens): exact counts to 2^53
        try:
            with torch.no_grad():
                for _ in range(batches):
                    x, y = self.data.next()
                    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.dtype == "bf16"):
                        doc_ids = None
                        if self.doc_len is not None:
                            from ..ops.attention import doc_ids_from_eos
                            doc_ids = doc_ids_from_eos(x, self.eos_id)
                        if self.fused_head:  # the head and the sums over row chunks (no DDP hooks under no_grad)
                            s, n = linear_cross_entropy_sums(self.module.hidden(x, doc_ids), self.module.output,
                                                             self._targets(x, y), ignore_index=self._ignore_index())
                        else:
                            out = self.net(x, doc_ids=doc_ids) if doc_ids is not None else self.net(x)
                            s, n = cross_entropy_sums(out.view(-1, out.shape[-1]), self._targets(x, y).view(-1),
                                                      ignore_index=self._ignore_index())
                    acc[0] += s
                    acc[1] += n
        finally:
            self.net.train(was_training)
        total, tokens = acc.tolist()  # the one read-back
        tokens = int(tokens)
        mean = total / max(tokens, 1)
        return {"nll": mean, "ppl": math.exp(mean) if mean < 700 else math.inf, "tokens": tokens}

    def last_loss(self) -> float:
        return float(self.loss.item()) if self.loss is not None else float("nan")

    def tokens_per_step(self) -> int:
        return self.B * (self.data.tokens.shape[1] - 1) if self.is_lm else self.B
