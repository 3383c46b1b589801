"""SD3Transformer2DModel — the MI355X-native trained component for the SD3 MMDiT (joint transformer blocks).

Mirrors the reference's module surface (simpletuner/helpers/models/sd3/transformer.py:244-911): same constructor arguments,
`forward(hidden_states[B,16,H,W], encoder_hidden_states, pooled_projections, timestep (0..1000), return_dict)` contract, the
diffusers state-dict keys (`pos_embed.proj.weight` stays the Conv2d [D,C,p,p] tensor; `pos_embed.pos_embed` the sincos buffer),
`.config`, `.parameters()`.  Forward and the hand-written backward are sequences of libst355 launches — the same kernels as
the Flux double block at D = 1536 / head_dim 64:
  * PatchEmbed = 2x2 patchify (im2col order) + ONE GEMM whose epilogue adds bias and the centre-cropped position table;
  * joint attention over [sample || context] (sd3 order, `JointAttnProcessor2_0`), no RoPE (identity tables), optional q/k RMSNorm;
  * the last block is `context_pre_only`: its context stream only feeds K/V/Q (AdaLayerNormContinuous, chunk order scale,shift);
  * every AdaLN modulation linear of all blocks (+norm_out) is one matrix -> one skinny GEMM per step;
  * unpatchify "nhwpqc->nchpwq" is the order-1 permute kernel.
Two training modes: frozen-base LoRA (`add_lora_adapter`) and the full fine-tune of BASELINE.json configs[3] (`enable_full_finetune`: TN weight-gradient
GEMMs, token-axis reductions for the modulation rows, q / k RMSNorm weight gradients; `_engine_backward_full`).
"""
from __future__ import annotations

import math
import os
from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from .. import ops
from ..engine import (IG_NAMES, NEXTLAT_NAMES, SELF_FLOW_NAMES, ST_NAMES, SelfTranscendenceHead, SelfTranscendenceTap, self_transcendence_indices, self_transcendence_shapes, AdapterArena, CaptureTap, SelfFlowHead, SelfFlowTap, self_flow_indices, self_flow_shapes, ArenaModule, FullGrads, InternalGuidanceHead, InternalGuidanceTap, LayerSyncTap, LokrGroup, LoraDropout, LoraGroup, NextLatHead, TLora,
                      NextLatTap, compact, frozen, internal_guidance_index, internal_guidance_shapes, layersync_indices, lin_w, lin_wT, lokr_init_norm, lora_down, lora_dx_finish, lora_dx_kw,
                      lora_fwd_kw, lora_grads, lora_pairs, lora_up, nextlat_index, node_backward, nextlat_init_reference, nextlat_shapes, pad64_empty, problems, rows_of, sincos_2d_hw)
from ..ops import EPI_ADD, EPI_GATE_RESIDUAL, EPI_GELU, EPI_MUL_GELU_GRAD
from ..training.checkpoint_plan import CheckpointPlanMixin

BF16 = torch.bfloat16
F32 = torch.float32
_BLOCK_ABI = os.environ.get("ST355_BLOCK_ABI", "1") != "0"      # A/B switch: 0 = sequence the blocks' kernels from the host instead of st355_block_sd3_joint_*


def sincos_2d(embed_dim: int, grid_size: int, base_size: int, interpolation_scale: float = 1.0) -> torch.Tensor:
    """diffusers get_2d_sincos_pos_embed: [grid_size^2, embed_dim] fp32 (w axis first, sin then cos per axis)"""
    return sincos_2d_hw(embed_dim, grid_size, grid_size, base_size, interpolation_scale)


def _stream_problems(B: int, S: int, rows: int, pr: dict, after: Optional[list] = None):
    """one projection over the `rows`-row block of every sample as ONE problem: segmented operands when the block is tile-aligned (the 4096 image rows,
    engine.problems); otherwise (the 154 text rows) through compact copies of the joint-buffer operands — the rows are gathered before the
    GEMM, a joint-buffer `out` is written to a compact temporary and scattered back by the closures appended to `after` (run them once the launch is
    issued).  A few MB of copies instead of B tiny launches per projection (measured: the per-sample form of the text stream cost as much as the image
    stream's segmentation saved)."""
    if B == 1 or rows % 256 == 0 or after is None or rows >= 1024:       # big unaligned blocks (odd aspect buckets): one problem per sample beats copying them
        return problems(B, rows, pr)
    q = dict(pr)
    for k in ("a", "a2", "aux_in"):
        v = q.get(k)
        if torch.is_tensor(v) and v.dim() == 3:
            q[k] = v.reshape(B * rows, v.shape[-1])                         # gather (copy)
    for k in ("out", "aux_out"):
        v = q.get(k)
        if torch.is_tensor(v) and v.dim() == 3:
            tmp = torch.empty(B * rows, v.shape[-1], dtype=v.dtype, device=v.device)
            q[k] = tmp
            after.append(lambda dst=v, src=tmp: dst.copy_(src.view(B, rows, -1)))      # scatter back into the joint rows
    return [q]


class SD3Transformer2DModel(CheckpointPlanMixin, ArenaModule):
    def __init__(self, sample_size: int = 128, patch_size: int = 2, in_channels: int = 16, num_layers: int = 18,
                 attention_head_dim: int = 64, num_attention_heads: int = 18, joint_attention_dim: int = 4096,
                 caption_projection_dim: int = 1152, pooled_projection_dim: int = 2048, out_channels: int = 16,
                 pos_embed_max_size: int = 96, dual_attention_layers: Tuple[int, ...] = (), qk_norm: Optional[str] = None,
                 internal_guidance_block_index: Optional[int] = None, nextlat_block_index: Optional[int] = None, device=None, **_ignored):
        super().__init__()
        # Internal Guidance (set_internal_guidance): given here, the head's four tensors get their place in the base parameter arena (what a full fine-tune trains)
        self._ig_block = None if internal_guidance_block_index is None else internal_guidance_index(internal_guidance_block_index, num_layers)
        self._ig_arena, self._ig = None, None
        # NextLat (set_nextlat): given here (the reference's rule: None / 0 / negative = the last block), the predictor's six tensors get their place in the base
        # parameter arena
        self._nl_block = None if nextlat_block_index is None else nextlat_index(nextlat_block_index, num_layers)
        self._nl_arena, self._nl, self._nl_mode, self._nl_loaded = None, None, "smooth_l1", False
        if self._ig_block is not None and self._nl_block is not None:
            raise NotImplementedError("Internal Guidance together with NextLat is not built on the st355 path (both heads claim the tail of the arena that trains)")
        if patch_size != 2:
            raise ValueError("patch_size must be 2 (the patchify kernels are 2x2)")
        self.dual_layers = frozenset(int(i) for i in (dual_attention_layers or ()))
        if any(i < 0 or i >= num_layers - 1 for i in self.dual_layers):
            raise ValueError("dual_attention_layers must name regular (not context_pre_only) blocks")      # sd3/transformer.py:295: the last block never is
        if attention_head_dim not in (64, 128):
            raise ValueError("attention_head_dim must be 64 or 128 (kernels built for these)")
        if qk_norm not in (None, "rms_norm"):
            raise ValueError("qk_norm must be None or 'rms_norm'")
        self.H, self.hd = num_attention_heads, attention_head_dim
        self.D = D = self.H * self.hd
        self.inner_dim = D
        if caption_projection_dim != D:
            raise ValueError("caption_projection_dim must equal num_attention_heads * attention_head_dim")
        self.config = SimpleNamespace(sample_size=sample_size, patch_size=patch_size, in_channels=in_channels, num_layers=num_layers,
                                      attention_head_dim=attention_head_dim, num_attention_heads=num_attention_heads,
                                      joint_attention_dim=joint_attention_dim, caption_projection_dim=caption_projection_dim,
                                      pooled_projection_dim=pooled_projection_dim, out_channels=out_channels,
                                      pos_embed_max_size=pos_embed_max_size, dual_attention_layers=tuple(sorted(self.dual_layers)), qk_norm=qk_norm)
        self.out_channels = out_channels
        if D % 64 or joint_attention_dim % 64 or pooled_projection_dim % 64 or (4 * in_channels) % 64:
            raise ValueError("all contraction dims must be multiples of 64")
        self.device_ = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        dev = self.device_
        # every weight / bias / modulation row is a view of ONE bf16 arena (allocation order = arena order): the full fine-tune then
        # has one gradient arena of the same layout, ONE fused optimizer launch and contiguous slices for the RCCL all-reduce.
        # Pass 1 counts (meta tensors), pass 2 hands out the views.
        self._build_arena(dev)
        self.pos_embed.register_buffer("pos_embed", torch.zeros(1, pos_embed_max_size * pos_embed_max_size, D, dtype=F32, device=dev))

        self.lora_groups: List[LoraGroup] = []
        self.lora_dropout: Optional[LoraDropout] = None          # add_lora_adapter(dropout > 0): applies to training forwards only
        self.lora_dora = False                                   # add_lora_adapter(dora=True): part of the weight, applies to every forward
        self.lora_lokr = False                                   # add_lokr_adapter(): LyCORIS LoKr, part of the weight, applies to every forward
        self.lokr_multiplier, self.lokr_validation_strength = 1.0, 1.0          # (the validation strength is `validation_lycoris_strength`: LoKr's and T-LoRA's)
        self.lora_tlora: Optional[TLora] = None                  # add_tlora_adapter(): LyCORIS T-LoRA, a per-sample rank mask from the timestep in every forward
        self.tlora_multiplier = 1
        self.lora_flat: Optional[torch.Tensor] = None
        self.lora_grad_flat: Optional[torch.Tensor] = None
        self._lora_params: List[nn.Parameter] = []
        self._cache: Dict = {}
        self._prepared = False
        self.accumulate_lora_grads = False
        self.gradient_checkpointing = False
        self.gradient_checkpointing_interval = None
        self.gradient_checkpointing_segment_stride = None
        self._tread_router, self._tread_routes = None, None
        self._layersync = None           # set_layersync(): 0-based (student, teacher) joint-block indices
        # Self-Flow (set_self_flow): the 0-based student / teacher blocks, the projector at the tail of the adapter arena, the teacher features of the next training forward
        self._sf_block, self._sf_teacher_block, self._sf, self._sf_feats, self._sf_tap = None, None, None, None, None
        # Self-Transcendence (set_self_transcendence): its settings, the projector at the tail of the adapter arena, the (target, sigmas) of the next training forward
        self._st_cfg, self._st, self._st_in = None, None, None
        self.grad_sync = None
        self._last_grad_flat = None
        self.full = False

    def _build(self):
        c = self.config
        D, dev, e = self.D, self.device_, self._alloc
        in_channels, out_channels, num_layers, qk_norm = c.in_channels, c.out_channels, c.num_layers, c.qk_norm
        joint_attention_dim, pooled_projection_dim = c.joint_attention_dim, c.pooled_projection_dim

        def lin(name, out_f, in_f):
            w, b = e(out_f, in_f), e(out_f)
            self._reg(name + ".weight", frozen(w)); self._reg(name + ".bias", frozen(b))
            return SimpleNamespace(w=w, b=b, wT=None, lora=None)

        # PatchEmbed: the Conv2d weight keeps its checkpoint shape; the GEMM reads it as [D, C*p*p]
        conv_w, conv_b = e(D, in_channels, 2, 2), e(D)
        self._reg("pos_embed.proj.weight", frozen(conv_w)); self._reg("pos_embed.proj.bias", frozen(conv_b))
        self.l_patch = SimpleNamespace(w=conv_w.view(D, 4 * in_channels), b=conv_b)
        self.l_t1 = lin("time_text_embed.timestep_embedder.linear_1", D, 256)
        self.l_t2 = lin("time_text_embed.timestep_embedder.linear_2", D, D)
        self.l_p1 = lin("time_text_embed.text_embedder.linear_1", D, pooled_projection_dim)
        self.l_p2 = lin("time_text_embed.text_embedder.linear_2", D, D)
        self.l_ctx = lin("context_embedder", D, joint_attention_dim)

        # last block: norm1_context is AdaLayerNormContinuous (2D); a dual-attention block's norm1 is SD35AdaLayerNormZeroX (9 chunks instead of 6)
        self.mod_total = (num_layers * 12 - 4 + 2 + 3 * len(self.dual_layers)) * D
        self.mod_w, self.mod_b = e(self.mod_total, D), e(self.mod_total)
        off = 0

        def mod_slice(name, n):
            nonlocal off
            self._reg(name + ".weight", frozen(self.mod_w[off:off + n])); self._reg(name + ".bias", frozen(self.mod_b[off:off + n]))
            o = off
            off += n
            return o

        def fused(prefix, names, out_each, in_f):
            n = len(names)
            w, b = e(n * out_each, in_f), e(n * out_each)
            for j, nm in enumerate(names):
                self._reg(f"{prefix}{nm}.weight", frozen(w[j * out_each:(j + 1) * out_each]))
                self._reg(f"{prefix}{nm}.bias", frozen(b[j * out_each:(j + 1) * out_each]))
            return SimpleNamespace(w=w, b=b, wT=None, lora=None)

        def normw(name):
            if qk_norm is None:
                return None
            w = e(self.hd)
            if not self._counting:
                w.fill_(1.0)
            self._reg(name + ".weight", frozen(w))
            return w

        self.blocks: List[SimpleNamespace] = []
        self._blocks_arena_lo = self._arena_numel
        for i in range(num_layers):
            p = f"transformer_blocks.{i}."
            blk = SimpleNamespace(last=(i == num_layers - 1), arena_lo=self._arena_numel, dual=(i in self.dual_layers))
            blk.mod_off = mod_slice(p + "norm1.linear", (9 if blk.dual else 6) * D)
            blk.mod_off_c = mod_slice(p + "norm1_context.linear", (2 if blk.last else 6) * D)
            blk.qkv = fused(p + "attn.", ["to_q", "to_k", "to_v"], D, D)
            blk.add_qkv = fused(p + "attn.", ["add_q_proj", "add_k_proj", "add_v_proj"], D, D)
            blk.to_out = fused(p + "attn.", ["to_out.0"], D, D)
            blk.to_add_out = None if blk.last else fused(p + "attn.", ["to_add_out"], D, D)
            blk.norm_q, blk.norm_k = normw(p + "attn.norm_q"), normw(p + "attn.norm_k")
            blk.norm_added_q, blk.norm_added_k = normw(p + "attn.norm_added_q"), normw(p + "attn.norm_added_k")
            # SD3.5 dual attention (sd3/transformer.py:155-165, 190-197): a second, image-only self-attention fed by the 7th-9th modulation chunks
            blk.qkv2 = fused(p + "attn2.", ["to_q", "to_k", "to_v"], D, D) if blk.dual else None
            blk.to_out2 = fused(p + "attn2.", ["to_out.0"], D, D) if blk.dual else None
            blk.norm_q2, blk.norm_k2 = (normw(p + "attn2.norm_q"), normw(p + "attn2.norm_k")) if blk.dual else (None, None)
            blk.ff1 = fused(p, ["ff.net.0.proj"], 4 * D, D)
            blk.ff2 = fused(p, ["ff.net.2"], D, 4 * D)
            blk.ffc1 = None if blk.last else fused(p, ["ff_context.net.0.proj"], 4 * D, D)
            blk.ffc2 = None if blk.last else fused(p, ["ff_context.net.2"], D, 4 * D)
            blk.arena_hi = self._arena_numel
            self.blocks.append(blk)
        self.mod_off_out = mod_slice("norm_out.linear", 2 * D)
        assert off == self.mod_total
        self._head_arena_lo = self._arena_numel
        self.l_out = lin("proj_out", 4 * out_channels, D)
        self._head_arena_hi = self._arena_numel
        if self._ig_block is not None:         # the Internal Guidance head, last in the arena: LayerNorm affine (1, 0), zero projection (internal_guidance.py:93-97)
            if 4 * out_channels != ops.IG_N:
                raise NotImplementedError(f"Internal Guidance: the head kernels are built for {ops.IG_N} output features (16 channels, 2 x 2 patch), got {4 * out_channels}")
            self._ig_arena = tuple(e(*shp) for shp in internal_guidance_shapes(D))
            for nm, t in zip(IG_NAMES, self._ig_arena):
                self._reg("internal_guidance_head." + nm, frozen(t))
            if not self._counting:
                self._ig_arena[0].fill_(1.0)
        if self._nl_block is not None:         # the NextLat predictor, last in the arena (nextlat.py:78-83: LayerNorm (1, 0), `up` as nn.Linear's default, `down` zero)
            self._nl_arena = tuple(e(*shp) for shp in nextlat_shapes(D))
            for nm, t in zip(NEXTLAT_NAMES, self._nl_arena):
                self._reg("nextlat_predictor." + nm, frozen(t))
            if not self._counting:
                self._nextlat_init_arena()

    # ------------------------------------------------------------------------------------------------
    # weights
    # ------------------------------------------------------------------------------------------------
    def _extra_state(self):
        return {"pos_embed.pos_embed": self.pos_embed.pos_embed}          # the position table: a buffer, saved and loaded with the parameters

    def _weights_changed(self):
        self._prepared = False
        self._cache.clear()

    @torch.no_grad()
    def init_synthetic(self, seed: int = 42):
        super().init_synthetic(seed)
        if self._ig_arena is not None:         # the head keeps the reference's initial values (registered last: the draws of every other parameter are unchanged)
            for t, v in zip(self._ig_arena, (1.0, 0.0, 0.0, 0.0)):
                t.fill_(v)
        if self._nl_arena is not None:         # (registered last as well)
            self._nextlat_init_arena()
        c = self.config
        self.pos_embed.pos_embed.copy_(sincos_2d(self.D, c.pos_embed_max_size, c.sample_size // c.patch_size)[None].to(self.device_))

    @torch.no_grad()
    def _nextlat_init_arena(self):
        """the reference's initial values for the arena's (bf16) predictor, from a generator of its own (the global one is left alone)"""
        nextlat_init_reference(self._nl_arena, self.D, torch.Generator(device=self.device_).manual_seed(1729))
        self._nl_loaded = False

    @torch.no_grad()
    def load_flat_state(self, state):
        super().load_flat_state(state)
        if self._nl_arena is not None and any(k.startswith("nextlat_predictor.") for k in state):
            self._nl_loaded = True                   # add_lora_adapter takes the file's predictor as the masters' start

    @torch.no_grad()
    def prepare_for_training(self):
        """K-major transposed copies for the dgrad GEMMs (frozen base => built once)"""
        for blk in self.blocks:
            for l in (blk.qkv, blk.add_qkv, blk.to_out, blk.to_add_out, blk.qkv2, blk.to_out2, blk.ff1, blk.ff2, blk.ffc1, blk.ffc2):
                if l is not None:
                    l.wT = l.w.t().contiguous()
        self.l_out.wT = self.l_out.w.t().contiguous()
        self._prepared = True

    # ------------------------------------------------------------------------------------------------
    # LoRA (peft naming), sd3/model.py:122 DEFAULT_LORA_TARGET = to_k,to_q,to_v,to_out.0
    # ------------------------------------------------------------------------------------------------
    def add_lora_adapter(self, rank: int = 32, alpha: Optional[float] = None, targets: str = "default", seed: int = 7, init_b_std: float = 0.0,
                         dropout: float = 0.0, dropout_seed: int = 0, dropout_rank: int = 0, dropout_calls: int = 0, dora: bool = False):
        """dropout: peft's `lora_dropout` (0 <= p < 1) — y = base(x) + (alpha / r) B A dropout(x) in training forwards, every adapted Linear with its own mask stream
        (its index in the ordered target list below); dropout_seed / dropout_rank make the mask key, dropout_calls is the call counter's start (engine.LoraDropout).
        dora: peft's `use_dora` — every adapted Linear gets a trainable magnitude vector m [out_features] (`<module>.lora_magnitude_vector.default.weight`, fp32, in
        the adapter arena right behind all A / B tensors) and computes y = (m / ||W + s B A||_row) . (x W^T + s (x A^T) B^T) + b, the norm detached; m starts as the
        norm of the freshly initialised adapter, so the first forward is the plain LoRA's (engine.LoraDora).  It applies to every forward, eval() included."""
        alpha = float(rank if alpha is None else alpha)
        dropout = float(dropout or 0.0)
        if not 0.0 <= dropout < 1.0:
            raise ValueError(f"lora_dropout must lie in [0, 1), got {dropout}")
        if dora and dropout > 0.0:
            raise NotImplementedError(f"use_dora with lora_dropout={dropout}: peft then feeds the dropped x to the base term of the DoRA correction, a different "
                                      "computation that is not built on the st355 path; set --lora_dropout=0 or --use_dora=false")
        D, dev = self.D, self.device_
        plan = []
        self.lora_groups = []
        self.lora_dropout = LoraDropout(dropout, dropout_seed, dropout_rank, dev, dropout_calls) if dropout > 0.0 else None
        self.lora_dora = bool(dora)
        group_lins = []

        def group(lin, prefix, names, K):
            g = LoraGroup(K, lin.w.shape[0], [(prefix + n, j * (lin.w.shape[0] // len(names)), lin.w.shape[0] // len(names))
                                              for j, n in enumerate(names)], rank, alpha, dev, streams=range(len(plan), len(plan) + len(names)))
            lin.lora = g
            self.lora_groups.append(g)
            group_lins.append(lin)
            for (name, n_off, N) in g.targets:
                plan.append((g, name, N, K))

        for i, blk in enumerate(self.blocks):
            p = f"transformer_blocks.{i}.attn."
            group(blk.qkv, p, ["to_q", "to_k", "to_v"], D)
            group(blk.to_out, p, ["to_out.0"], D)
            if blk.dual:       # peft matches target modules by suffix: attn2.to_q / to_k / to_v / to_out.0 carry adapters too
                p2 = f"transformer_blocks.{i}.attn2."
                group(blk.qkv2, p2, ["to_q", "to_k", "to_v"], D)
                group(blk.to_out2, p2, ["to_out.0"], D)
            if targets == "all":
                group(blk.add_qkv, p, ["add_q_proj", "add_k_proj", "add_v_proj"], D)
                if blk.to_add_out is not None:
                    group(blk.to_add_out, p, ["to_add_out"], D)
        arena = AdapterArena(self, dev)
        draw = lora_pairs(arena, plan, rank, init_b_std)
        # DoRA: the magnitudes follow all A / B tensors (flat_view of parameters and of gradients stays one run), before the heads
        mags = [[arena.add(name + ".lora_magnitude_vector.default.weight", (N,)) for (name, _, N) in g.targets] for g in self.lora_groups] if dora else []
        # Internal Guidance, then NextLat: the heads' fp32 masters follow the adapters in the same arena (one run for the optimizer), the predictor from a 16-byte
        # boundary (its kernels move 8 elements per lane)
        ig = [arena.add("internal_guidance_head." + nm, shp) for nm, shp in zip(IG_NAMES, internal_guidance_shapes(D))] if self._ig_block is not None else []
        nl = [arena.add("nextlat_predictor." + nm, shp, align=1 if k else 8) for k, (nm, shp) in enumerate(zip(NEXTLAT_NAMES, nextlat_shapes(D)))] \
            if self._nl_block is not None else []
        # Self-Flow: the projector's fp32 masters likewise (it excludes the two heads above), from a 16-byte boundary
        sf = [arena.add("crepa_projector." + nm, shp, align=1 if k else 8) for k, (nm, shp) in enumerate(zip(SELF_FLOW_NAMES, self_flow_shapes(D)))] \
            if self._sf_block is not None else []
        # Self-Transcendence: the projector's fp32 masters likewise (it excludes every head above)
        st = [arena.add("self_transcendence_projector." + nm, shp, align=1 if k else 8)
              for k, (nm, shp) in enumerate(zip(ST_NAMES, self_transcendence_shapes(D, self._st_cfg.hidden_dim)))] if self._st_cfg is not None else []
        if sf and dora:
            raise NotImplementedError("crepa_enabled (self_flow) with use_dora: the teacher forward packs the adapters from the EMA shadow, which the DoRA fold does not "
                                      "take; not built on the st355 path")
        gen = arena.build(seed)
        draw(gen)
        for g, lin, ms in zip(self.lora_groups, group_lins, mags):
            lo, hi = ms[0].lo, ms[-1].hi
            g.enable_dora(lin, self.lora_flat[lo:hi], self.lora_grad_flat[lo:hi], lo)
            g.pack()
            g.fold(init=True)                    # m = ||W + s B A||_row of the fresh adapter (peft's DoraLinearLayer.update_layer): g = 1 at step 0
        if ig:
            self._ig = InternalGuidanceHead(self._ig_block, D, [s.p for s in ig], [s.g for s in ig], ig[0].lo, ig[-1].hi, dev)
            self._ig.init_reference()
            if self._ig_arena is not None:
                for s, src in zip(ig, self._ig_arena):
                    s.p.copy_(src)               # a head that came with the loaded weights
        if nl:
            self._nl = NextLatHead(self._nl_block, D, [s.p for s in nl], [s.g for s in nl], nl[0].lo, nl[-1].hi, dev)
            if self._nl_arena is not None and self._nl_loaded:
                for s, src in zip(nl, self._nl_arena):
                    s.p.copy_(src)               # a predictor that came with the loaded weights
            else:
                self._nl.init_reference(gen)         # the reference's initial values, drawn in fp32 from the adapters' generator
        if sf:
            self._sf = SelfFlowHead(self._sf_block, self._sf_teacher_block, D, [s.p for s in sf], [s.g for s in sf], sf[0].lo, sf[-1].hi, dev)
            self._sf.init_reference(gen)             # nn.LayerNorm / nn.Linear defaults, drawn in fp32 from the adapters' generator behind every A / B draw
        if st:
            self._st = SelfTranscendenceHead(self._st_cfg.student_block, D, self._st_cfg.hidden_dim, [s.p for s in st], [s.g for s in st], st[0].lo, st[-1].hi, dev)
            self._st.init_reference(gen)             # nn.Linear's defaults, drawn in fp32 from the adapters' generator behind every A / B draw
        return self._lora_params

    # ------------------------------------------------------------------------------------------------
    # LyCORIS LoKr (`lora_type=lycoris`, `algo: lokr`): engine.LokrGroup on the Attention and FeedForward Linears
    # ------------------------------------------------------------------------------------------------
    LOKR_CLASSES = ("Attention", "FeedForward")

    def add_lokr_adapter(self, factors: Optional[Dict[str, int]] = None, multiplier: float = 1.0, seed: int = 7, init_norm: Optional[float] = None,
                         linear_dim: Optional[int] = None):
        """factors: {"Attention": factor, "FeedForward": factor} — the module classes that get adapters (LyCORIS' `target_module`) and their `factor`.  Every Linear of a
        selected class gets w1 [ol, im] and w2 [ok, in] (`<module>.lokr_w1` / `<module>.lokr_w2`, fp32, back to back in the adapter arena in target order) and
        computes y = x bf16(W + multiplier kron(w1, w2))^T + b in every forward, eval() included.  w1 ~ U(-1 / sqrt(im), 1 / sqrt(im)) and w2 = 0: the first
        forward is the base model's bit for bit.  init_norm (the `init_lokr_norm` value): w1 = 1 and w2 a normal draw rescaled to the frozen weight's norm, std and
        mean, times the value.  linear_dim: LyCORIS' rank bound — a value that would make any w2 low-rank is refused."""
        factors = dict(factors if factors is not None else {"Attention": 10, "FeedForward": 4})
        for k in factors:
            if k not in self.LOKR_CLASSES:
                raise NotImplementedError(f"lycoris lokr: target_module entry {k!r} is not built on the st355 path (built: {', '.join(self.LOKR_CLASSES)})")
        if self._st_cfg is not None:
            raise ValueError("Self-Transcendence supports full-model and standard PEFT LoRA training; LyCORIS is not supported.")
        if self._ig_block is not None or self._nl_block is not None or self._sf_block is not None:
            raise NotImplementedError("lycoris lokr with an Internal Guidance head / a NextLat predictor / a Self-Flow projector is not built on the st355 path")
        dev = self.device_
        self.lora_groups, self.lora_dropout, self.lora_dora, self.lora_lokr = [], None, False, True
        self.lokr_multiplier = float(multiplier)
        self.lokr_linear_dim = 10000 if linear_dim is None else int(linear_dim)          # what an adapter file records as `alpha`
        plan = []

        def group(lin, prefix, names, factor):
            n_each = lin.w.shape[0] // len(names)
            g = LokrGroup(lin, [(prefix + n, j * n_each, n_each) for j, n in enumerate(names)], [factor] * len(names), dev)
            lin.lora = g
            self.lora_groups.append(g)
            plan.append(g)

        fa, ff = factors.get("Attention"), factors.get("FeedForward")
        for i, blk in enumerate(self.blocks):
            p = f"transformer_blocks.{i}."
            if fa is not None:
                group(blk.qkv, p + "attn.", ["to_q", "to_k", "to_v"], fa)
                group(blk.to_out, p + "attn.", ["to_out.0"], fa)
                group(blk.add_qkv, p + "attn.", ["add_q_proj", "add_k_proj", "add_v_proj"], fa)
                if blk.to_add_out is not None:
                    group(blk.to_add_out, p + "attn.", ["to_add_out"], fa)
                if blk.dual:
                    group(blk.qkv2, p + "attn2.", ["to_q", "to_k", "to_v"], fa)
                    group(blk.to_out2, p + "attn2.", ["to_out.0"], fa)
            if ff is not None:
                group(blk.ff1, p, ["ff.net.0.proj"], ff)
                group(blk.ff2, p, ["ff.net.2"], ff)
                if blk.ffc1 is not None:
                    group(blk.ffc1, p, ["ff_context.net.0.proj"], ff)
                    group(blk.ffc2, p, ["ff_context.net.2"], ff)
        if linear_dim is not None:          # LyCORIS keeps w2 a full matrix only while linear_dim >= max(ok, in) / 2; below that it trains a low-rank pair
            for g in plan:
                for (name, _, _), (ol, ok, im, in_) in zip(g.targets, g.shapes):
                    if linear_dim < max(ok, in_) / 2:
                        raise NotImplementedError(f"lycoris_config linear_dim={linear_dim}: {name} would get a low-rank w2 ([{ok}, {in_}] needs linear_dim >= "
                                                  f"{max(ok, in_) // 2}), which is not built on the st355 path; set \"linear_dim\": 10000 (full matrices)")
        arena = AdapterArena(self, dev)
        slots = [[(arena.add(name + ".lokr_w1", (ol, im)), arena.add(name + ".lokr_w2", (ok, in_))) for (name, _, _), (ol, ok, im, in_) in zip(g.targets, g.shapes)] for g in plan]
        gen = arena.build(seed)
        for g, pairs in zip(plan, slots):
            g.flat_lo, g.flat_hi = pairs[0][0].lo, pairs[-1][1].hi
            for (name, n_off, N), (s1, s2) in zip(g.targets, pairs):
                if init_norm is None:
                    ol, im = s1.shape
                    s1.p.copy_((torch.rand(ol, im, generator=gen, device=dev) * 2 - 1) * (1.0 / math.sqrt(im)))
                else:
                    s1.p.fill_(1.0)
                    lokr_init_norm(g.lin.w[n_off:n_off + N], s2.p, float(init_norm), gen)
                g.w1.append(s1.p); g.w2.append(s2.p); g.g1.append(s1.g); g.g2.append(s2.g)
        return self._lora_params

    # ------------------------------------------------------------------------------------------------
    # LyCORIS T-LoRA (`lora_type=lycoris`, `algo: tlora`): engine.LoraGroup + engine.TLora on the LoKr site list
    # ------------------------------------------------------------------------------------------------
    TLORA_MAX_DIM = 128          # the largest rank the rank-space kernels are exercised at (LoraGroup walks ranks above 64 in 64-column slabs)

    def add_tlora_adapter(self, classes=("Attention", "FeedForward"), linear_dim: int = 4, linear_alpha: int = 1, multiplier: int = 1, min_rank: int = 1,
                          alpha: float = 1.0, num_train_timesteps: int = 1000, seed: int = 7):
        """classes: the module classes that get adapters (LyCORIS' `target_module`), on add_lokr_adapter's site list.  Every Linear of a selected class gets
        down [r, in] and up [out, r] (`<module>.lora_down.weight` / `<module>.lora_up.weight`, fp32, pair by pair in the adapter arena in target order; r = linear_dim)
        and computes, for sample b,  y_b = x_b W^T + bias + multiplier (linear_alpha / r) (mask_b . (x_b down^T)) up^T  in every forward, eval() included (there the
        multiplier is times `lokr_validation_strength`), mask_b = the first r_b rank columns, r_b = engine.tlora_active_rank(int(timestep_b), num_train_timesteps,
        r, min_rank, alpha).  LyCORIS' LoCon start: down ~ U(-1 / sqrt(in), 1 / sqrt(in)) (kaiming_uniform(a = sqrt 5)), up = 0 — the first forward is the base
        model's bit for bit.  multiplier, linear_dim and linear_alpha are taken through int(), as the reference does."""
        classes = list(classes)
        for k in classes:
            if k not in self.LOKR_CLASSES:
                raise NotImplementedError(f"lycoris tlora: target_module entry {k!r} is not built on the st355 path (built: {', '.join(self.LOKR_CLASSES)})")
        if self._st_cfg is not None:
            raise ValueError("Self-Transcendence supports full-model and standard PEFT LoRA training; LyCORIS is not supported.")
        if self._ig_block is not None or self._nl_block is not None or self._sf_block is not None:
            raise NotImplementedError("lycoris tlora with an Internal Guidance head / a NextLat predictor / a Self-Flow projector is not built on the st355 path")
        rank, a, mult = int(linear_dim), int(linear_alpha), int(multiplier)
        if not 1 <= rank <= self.TLORA_MAX_DIM:
            raise NotImplementedError(f"lycoris_config linear_dim={rank}: the rank-space kernels of the st355 path take 1 <= linear_dim <= {self.TLORA_MAX_DIM}; set "
                                      f"\"linear_dim\" inside that range")
        dev = self.device_
        state = TLora(rank, min_rank, alpha, num_train_timesteps, dev)          # (refuses tlora_min_rank / tlora_alpha outside their ranges)
        self.lora_groups, self.lora_dropout, self.lora_dora, self.lora_lokr, self.lora_tlora = [], None, False, False, state
        self.tlora_multiplier, self.tlora_linear_alpha = mult, a
        plan = []

        def group(lin, prefix, names):
            n_each = lin.w.shape[0] // len(names)
            g = LoraGroup(lin.w.shape[1], lin.w.shape[0], [(prefix + n, j * n_each, n_each) for j, n in enumerate(names)], rank, float(a), dev)
            g.tlora_scale = g.scale            # alpha / r; `scale` itself is set by every forward: times the multiplier (eval(): and the validation strength)
            g.scale = mult * g.tlora_scale
            lin.lora = g
            self.lora_groups.append(g)
            plan.append(g)

        for i, blk in enumerate(self.blocks):
            p = f"transformer_blocks.{i}."
            if "Attention" in classes:
                group(blk.qkv, p + "attn.", ["to_q", "to_k", "to_v"])
                group(blk.to_out, p + "attn.", ["to_out.0"])
                group(blk.add_qkv, p + "attn.", ["add_q_proj", "add_k_proj", "add_v_proj"])
                if blk.to_add_out is not None:
                    group(blk.to_add_out, p + "attn.", ["to_add_out"])
                if blk.dual:
                    group(blk.qkv2, p + "attn2.", ["to_q", "to_k", "to_v"])
                    group(blk.to_out2, p + "attn2.", ["to_out.0"])
            if "FeedForward" in classes:
                group(blk.ff1, p, ["ff.net.0.proj"])
                group(blk.ff2, p, ["ff.net.2"])
                if blk.ffc1 is not None:
                    group(blk.ffc1, p, ["ff_context.net.0.proj"])
                    group(blk.ffc2, p, ["ff_context.net.2"])
        arena = AdapterArena(self, dev)
        slots = [[(arena.add(name + ".lora_down.weight", (rank, g.K)), arena.add(name + ".lora_up.weight", (N, rank))) for (name, _, N) in g.targets] for g in plan]
        gen = arena.build(seed)
        for g, pairs in zip(plan, slots):
            g.flat_lo, g.flat_hi = pairs[0][0].lo, pairs[-1][1].hi
            for sd, su in pairs:
                sd.p.copy_((torch.rand(rank, g.K, generator=gen, device=dev) * 2 - 1) * (1.0 / math.sqrt(g.K)))
                g.A.append(sd.p); g.B.append(su.p); g.gA.append(sd.g); g.gB.append(su.g)
        return self._lora_params

    # ------------------------------------------------------------------------------------------------
    def _tables(self, h: int, w: int, S: int, B: int):
        """cropped position table expanded over the batch ([B*h*w, D] bf16) and identity RoPE tables (SD3 has no RoPE)"""
        key = (h, w, S, B)
        hit = self._cache.get(key)
        if hit is None:
            mx = self.config.pos_embed_max_size
            if h > mx or w > mx:
                raise ValueError(f"latent grid {h}x{w} exceeds pos_embed_max_size {mx}")
            top, left = (mx - h) // 2, (mx - w) // 2
            pos = self.pos_embed.pos_embed[0].view(mx, mx, self.D)[top:top + h, left:left + w].reshape(h * w, self.D).to(BF16)
            pos = pos[None].expand(B, -1, -1).reshape(B * h * w, self.D).contiguous()
            cos = torch.ones(S, self.hd, dtype=F32, device=self.device_); sin = torch.zeros(S, self.hd, dtype=F32, device=self.device_)
            hit = (pos, cos, sin)
            self._cache[key] = hit
        return hit

    def _block_fwd(self, blk, img, txt, env, save: bool):
        """one JointTransformerBlock (sd3/transformer.py:145-241 `_sd3_apply_joint_transformer_block`): returns (img', txt' | None, saved activations | None).
        Also the RECOMPUTE unit of the activation-checkpoint plans (training/checkpoint_plan.py): run again from a segment's kept input in backward, it
        launches the same kernels in the same order on the same values — bit-identical activations, hence bit-identical gradients."""
        D, H, hd, dev = self.D, self.H, self.hd, self.device_
        B, Si, St, S, Sp, cos, sin, mod, scale, full = env.B, env.Si, env.St, env.S, env.Sp, env.cos, env.sin, env.mod, env.scale, env.full
        ybuf = (lambda rows: torch.empty(rows, D, dtype=BF16, device=dev)) if (full and save) else (lambda rows: None)
        rpb = 1 if env.rpb_i == 1 else Si     # rows of the image stream that share one modulation row: the sample's (inside a TREAD route: its kept) rows, or 1 under tokenwise timesteps
        drop = getattr(env, "drop", None)      # LoRA dropout of this training forward (and of its recompute passes): the adapters' down projections draw masks
        tl = getattr(env, "tl", None)          # T-LoRA: this forward's timesteps bound to the rank table — every down projection is masked per sample behind its product
        if self._c_entry_ok(blk, env, (img, txt), full=full, backward=False):
            return self._block_fwd_c(blk, img, txt, env, save, ybuf)

        mi = env.mod_i[:, blk.mod_off:blk.mod_off + 6 * D]
        n_img = ops.ln_modulate_fwd(img, mi[:, D:2 * D], mi[:, :D], rpb)
        if blk.last:
            mt = mod[:, blk.mod_off_c:blk.mod_off_c + 2 * D]
            n_txt = ops.ln_modulate_fwd(txt, mt[:, :D], mt[:, D:2 * D], St)          # AdaLayerNormContinuous: (scale, shift)
        else:
            mt = mod[:, blk.mod_off_c:blk.mod_off_c + 6 * D]
            n_txt = ops.ln_modulate_fwd(txt, mt[:, D:2 * D], mt[:, :D], St)
        qkv = torch.empty(B * S, 3 * D, dtype=BF16, device=dev)
        T_img, T_txt = lora_down(blk.qkv, n_img, drop, tl=tl), lora_down(blk.add_qkv, n_txt, drop, tl=tl)
        # the image stream (4096 rows per sample: tile-aligned) is ONE segmented problem over the joint buffer; the 154 text rows stay per sample
        after = []
        ops.gemm_grouped(_stream_problems(B, S, Si, dict(a=n_img, w=lin_w(blk.qkv), bias=blk.qkv.b, out=rows_of(qkv, 0, Si, B, S), **lora_fwd_kw(blk.qkv, T_img)), after)
                         + _stream_problems(B, S, St, dict(a=n_txt, w=lin_w(blk.add_qkv), bias=blk.add_qkv.b, out=rows_of(qkv, Si, St, B, S),
                                                           **lora_fwd_kw(blk.add_qkv, T_txt)), after))
        for f in after:
            f()
        Q = torch.empty(B, H, S, hd, dtype=BF16, device=dev); K = torch.empty_like(Q)
        mk = torch.zeros if Sp > S else torch.empty
        # head-major Q^T / K^T copies only for the copy-reading backward kernels (ST355_ATTN_TR=0); the default backward gathers those fragments by
        # transposing LDS reads from the row-major tiles (attention_bwd.hip dkv3 / dq<TR>, r3: head_dim 64 too)
        Qt = Kt = None
        if not ops.ATTN_TR:
            Qt = mk(B, H, hd, Sp, dtype=BF16, device=dev); Kt = mk(B, H, hd, Sp, dtype=BF16, device=dev)
        Vt = mk(B, H, hd, Sp, dtype=BF16, device=dev)
        ops.qk_norm_rope_fwd(qkv, blk.norm_q, blk.norm_k, cos, sin, Q, K, Qt, Kt, Vt, B, H, hd, Si, 0, S, Sp)
        ops.qk_norm_rope_fwd(qkv, blk.norm_added_q, blk.norm_added_k, cos, sin, Q, K, Qt, Kt, Vt, B, H, hd, St, Si, S, Sp)
        O = torch.empty(B * S, D, dtype=BF16, device=dev); lse2 = torch.empty(B, H, S, dtype=F32, device=dev)
        ops.attn_fwd(Q, K, Vt, O, lse2, B, H, S, Sp, hd, scale)
        del Vt
        x1_img = torch.empty(B * Si, D, dtype=BF16, device=dev)
        x1_txt = None if blk.last else torch.empty(B * St, D, dtype=BF16, device=dev)
        ya_i, ya_t = ybuf(B * Si), (None if blk.last else ybuf(B * St))
        O_i, O_t = rows_of(O, 0, Si, B, S), rows_of(O, Si, St, B, S)
        after = []
        if B > 1 and St % 256:
            O_t = O_t.reshape(B * St, D)                                  # the text rows of the attention output, gathered once for both uses below

        def down_rows(lin, x, rows):
            """lora_down over one stream's rows of the joint attention output: undropped, the plain GEMM in the operand form of the projection itself"""
            if lin is None or lin.lora is None or not lin.lora.K2:          # (a LoKr group has no rank-space side path)
                return None
            T = torch.empty(B * rows, lin.lora.K2, dtype=BF16, device=dev)
            if drop is not None:
                lora_down(lin, x, drop, out=T)                            # (the view as it is: the mask follows the logical row b * rows + s)
            else:
                for pr in _stream_problems(B, S, rows, dict(a=x, w=lin.lora.A_cat, out=T), after):
                    ops.gemm(pr.pop("a"), pr.pop("w"), **pr)
                if tl is not None:
                    lin.lora.tlora_mask(T, tl)
            return T

        aux = lambda y: {} if y is None else dict(aux_out=y)
        T_o = down_rows(blk.to_out, O_i, Si)
        probs = _stream_problems(B, S, Si, dict(a=O_i, w=lin_w(blk.to_out), bias=blk.to_out.b, out=x1_img, epilogue=EPI_GATE_RESIDUAL, aux_in=img,
                                                gate=mi[:, 2 * D:3 * D], rows_per_batch=rpb, **aux(ya_i), **lora_fwd_kw(blk.to_out, T_o)), after)
        T_ao = down_rows(blk.to_add_out, O_t, St)                         # (a context_pre_only block has no to_add_out)
        if not blk.last:
            probs += _stream_problems(B, S, St, dict(a=O_t, w=lin_w(blk.to_add_out), bias=blk.to_add_out.b, out=x1_txt, epilogue=EPI_GATE_RESIDUAL,
                                                     aux_in=txt, gate=mt[:, 2 * D:3 * D], rows_per_batch=St, **aux(ya_t), **lora_fwd_kw(blk.to_add_out, T_ao)), after)
        ops.gemm_grouped(probs)
        for f in after:
            f()
        d2 = None
        if blk.dual:
            # attn2: self-attention over the image tokens only, input = LN(img) modulated by chunks 7 / 8 (shift_msa2, scale_msa2), residual gated by chunk 9
            # onto the stream AFTER the joint-attention residual (sd3/transformer.py:190-197)
            mi9 = mod[:, blk.mod_off:blk.mod_off + 9 * D]                        # (dual blocks never run tokenwise: refused in _engine_forward)
            Sip = (Si + 63) // 64 * 64
            n2a = ops.ln_modulate_fwd(img, mi9[:, 7 * D:8 * D], mi9[:, 6 * D:7 * D], Si)
            T2 = lora_down(blk.qkv2, n2a, drop, tl=tl)
            qkv2 = ops.gemm(n2a, lin_w(blk.qkv2), bias=blk.qkv2.b, **lora_fwd_kw(blk.qkv2, T2))
            Q2 = torch.empty(B, H, Si, hd, dtype=BF16, device=dev); K2 = torch.empty_like(Q2)
            mk2 = torch.zeros if Sip > Si else torch.empty
            Q2t = K2t = None
            if not ops.ATTN_TR:
                Q2t = mk2(B, H, hd, Sip, dtype=BF16, device=dev); K2t = mk2(B, H, hd, Sip, dtype=BF16, device=dev)
            V2t = mk2(B, H, hd, Sip, dtype=BF16, device=dev)
            ops.qk_norm_rope_fwd(qkv2, blk.norm_q2, blk.norm_k2, cos, sin, Q2, K2, Q2t, K2t, V2t, B, H, hd, Si, 0, Si, Sip)
            O2 = torch.empty(B * Si, D, dtype=BF16, device=dev); lse2b = torch.empty(B, H, Si, dtype=F32, device=dev)
            ops.attn_fwd(Q2, K2, V2t, O2, lse2b, B, H, Si, Sip, hd, scale)
            del V2t
            ya2 = ybuf(B * Si)
            T_o2 = lora_down(blk.to_out2, O2, drop, tl=tl)
            x1b_img = ops.gemm(O2, lin_w(blk.to_out2), bias=blk.to_out2.b, epilogue=EPI_GATE_RESIDUAL, aux_in=x1_img, gate=mi9[:, 8 * D:9 * D], rows_per_batch=Si,
                               **aux(ya2), **lora_fwd_kw(blk.to_out2, T_o2))
            d2 = SimpleNamespace(n2a=n2a, qkv2=qkv2, T2=T2, Q2=Q2, K2=K2, Q2t=Q2t, K2t=K2t, O2=O2, lse2b=lse2b, ya2=ya2, T_o2=T_o2, Sip=Sip)
            x1_img = x1b_img                       # what the MLP branch (and its residual) sees
        n2_i = ops.ln_modulate_fwd(x1_img, mi[:, 4 * D:5 * D], mi[:, 3 * D:4 * D], rpb)
        hpre_img = torch.empty(B * Si, 4 * D, dtype=BF16, device=dev)
        hpre_txt = x2_txt = n2_t = h_t = None
        yf_i, yf_t = ybuf(B * Si), (None if blk.last else ybuf(B * St))
        kf_i, kf_t = aux(yf_i), aux(yf_t)
        # the feed-forward Linears' rank-space adapters (T-LoRA's FeedForward sites; nothing for a LoKr group or without an adapter): T = x A^T, masked, then the
        # K-extension of the projection's own launch, in front of its GELU / gated-residual epilogue
        T_f1 = T_f2 = T_c1 = T_c2 = None
        if blk.last:
            T_f1 = lora_down(blk.ff1, n2_i, drop, tl=tl)
            h_i = ops.gemm(n2_i, lin_w(blk.ff1), bias=blk.ff1.b, epilogue=EPI_GELU, aux_out=hpre_img, **lora_fwd_kw(blk.ff1, T_f1))
            T_f2 = lora_down(blk.ff2, h_i, drop, tl=tl)
            x2_img = ops.gemm(h_i, lin_w(blk.ff2), bias=blk.ff2.b, epilogue=EPI_GATE_RESIDUAL, aux_in=x1_img, gate=mi[:, 5 * D:6 * D],
                              rows_per_batch=rpb, **kf_i, **lora_fwd_kw(blk.ff2, T_f2))
        else:
            n2_t = ops.ln_modulate_fwd(x1_txt, mt[:, 4 * D:5 * D], mt[:, 3 * D:4 * D], St)
            hpre_txt = torch.empty(B * St, 4 * D, dtype=BF16, device=dev)
            T_f1, T_c1 = lora_down(blk.ff1, n2_i, drop, tl=tl), lora_down(blk.ffc1, n2_t, drop, tl=tl)
            h_i, h_t = ops.gemm_grouped([dict(a=n2_i, w=lin_w(blk.ff1), bias=blk.ff1.b, epilogue=EPI_GELU, aux_out=hpre_img, **lora_fwd_kw(blk.ff1, T_f1)),
                                         dict(a=n2_t, w=lin_w(blk.ffc1), bias=blk.ffc1.b, epilogue=EPI_GELU, aux_out=hpre_txt, **lora_fwd_kw(blk.ffc1, T_c1))])
            T_f2, T_c2 = lora_down(blk.ff2, h_i, drop, tl=tl), lora_down(blk.ffc2, h_t, drop, tl=tl)
            x2_img, x2_txt = ops.gemm_grouped([
                dict(a=h_i, w=lin_w(blk.ff2), bias=blk.ff2.b, epilogue=EPI_GATE_RESIDUAL, aux_in=x1_img, gate=mi[:, 5 * D:6 * D], rows_per_batch=rpb, **kf_i,
                     **lora_fwd_kw(blk.ff2, T_f2)),
                dict(a=h_t, w=lin_w(blk.ffc2), bias=blk.ffc2.b, epilogue=EPI_GATE_RESIDUAL, aux_in=x1_txt, gate=mt[:, 5 * D:6 * D], rows_per_batch=St, **kf_t,
                     **lora_fwd_kw(blk.ffc2, T_c2))])
        if save:
            sv = SimpleNamespace(img=img, txt=txt, n_img=n_img, n_txt=n_txt if (blk.add_qkv.lora is not None or full) else None, qkv=qkv, Q=Q, K=K,
                                 Qt=Qt, Kt=Kt, O=O, lse2=lse2, x1_img=x1_img, x1_txt=x1_txt, hpre_img=hpre_img,
                                 hpre_txt=hpre_txt, T_img=T_img, T_txt=T_txt, T_o=T_o, T_ao=T_ao, d2=d2, T_f1=T_f1, T_f2=T_f2, T_c1=T_c1, T_c2=T_c2)
            if full:    # a full fine-tune also needs every Linear's input (weight gradients) and the un-gated branch outputs (gate gradients)
                sv.n2_i, sv.n2_t, sv.h_i, sv.h_t, sv.ya_i, sv.ya_t, sv.yf_i, sv.yf_t = n2_i, n2_t, h_i, h_t, ya_i, ya_t, yf_i, yf_t
            return x2_img, x2_txt, sv
        return x2_img, x2_txt, None

    @staticmethod
    def _lk(lin):
        """(K2, k2_real, A_cat, B_blk, A_cat_T, B_blk_T) of a Linear's adapter group, zeros / None without one"""
        g = lin.lora if lin is not None else None
        if g is None:
            return 0, 0, None, None, None, None
        return g.K2, getattr(g, "k2_real", 0), g.A_cat, g.B_blk, g.A_cat_T, g.B_blk_T

    def _c_entry_ok(self, blk, env, streams, *, full: bool, backward: bool, sv=None) -> bool:
        """may this block go through its C entry (st355_block_sd3_joint_fwd / _bwd) instead of the host-sequenced form?  `streams`: the (img, txt) inputs of the
        forward, the (d_img, d_txt | None) gradients of the backward.  Every form: the switch is on, a regular block (the entries know no attn2), the
        transposing-LDS attention backward (the entries keep no head-major Q^T / K^T copies), contiguous streams (they take plain pointers).
          forward                 one modulation row per sample (rpb == Si; tokenwise timesteps index it per token), no LoRA dropout and no DoRA (the entries
                                  sequence neither the masked rank-space kernels nor the folded operands)
          backward                the activations come from a forward that kept no Q^T / K^T (sv.Qt is None)
          backward, LoRA          as the forward, the tokenwise test on the step's own rows-per-batch (rpb != 1)
          backward, full          no trainable q / k RMSNorm weights (SD3.5): their gradients ride in the host form's RMSNorm backward pass"""
        if not (_BLOCK_ABI and not blk.dual and ops.ATTN_TR and all(t is None or t.is_contiguous() for t in streams)):
            return False
        # (T-LoRA: the entries fuse the unmasked rank-space products and know no feed-forward adapter sites)
        plain_lora = getattr(env, "drop", None) is None and not self.lora_dora and not self.lora_lokr and self.lora_tlora is None
        if not backward:
            return (1 if env.rpb_i == 1 else env.Si) == env.Si and plain_lora
        if not full:
            return sv.Qt is None and env.rpb_i != 1 and plain_lora
        return sv.Qt is None and blk.norm_q is None and blk.norm_k is None and blk.norm_added_q is None and blk.norm_added_k is None

    def _block_fwd_c(self, blk, img, txt, env, save: bool, ybuf):
        """_block_fwd through st355_block_sd3_joint_fwd: ONE C call sequences the launches of the host-side form below on the same operands —
        every buffer is allocated here and the kept ones go to the backward as before; bit-identical to it (ST355_BLOCK_ABI=0 restores the host sequencing)."""
        D, H, hd, dev = self.D, self.H, self.hd, self.device_
        B, Si, St, S, Sp, mod, full = env.B, env.Si, env.St, env.S, env.Sp, env.mod, env.full
        e = lambda *sh, dt=BF16: torch.empty(*sh, dtype=dt, device=dev)
        last = blk.last
        K2q, kr_q, A_q, Bb_q, _, _ = self._lk(blk.qkv)
        K2a, kr_a, A_a, Bb_a, _, _ = self._lk(blk.add_qkv)
        K2o, kr_o, A_o, Bb_o, _, _ = self._lk(blk.to_out)
        K2t, kr_t, A_t, Bb_t, _, _ = self._lk(None if last else blk.to_add_out)
        et = (lambda r, c: pad64_empty(r, c, dev)) if (full and save) else e        # text-stream tensors a full fine-tune contracts over tokens: zero-tailed to 64 rows
        n_img, n_txt, qkv, O, x1_img, hpre_img, n2_i, h_i, x2_img = (e(B * Si, D), et(B * St, D), e(B * S, 3 * D), e(B * S, D), e(B * Si, D), e(B * Si, 4 * D),
                                                                     e(B * Si, D), e(B * Si, 4 * D), e(B * Si, D))
        Q, K, lse2 = e(B, H, S, hd), e(B, H, S, hd), e(B, H, S, dt=F32)
        Vt = e(B, H, hd, Sp)
        if Sp > S:
            Vt[..., S:].zero_()                                 # only the pad columns need the zeros (the rest is written by the re-layout pass)
        x1_txt = hpre_txt = n2_t = h_t = x2_txt = None
        if not last:
            x1_txt, hpre_txt, n2_t, h_t, x2_txt = e(B * St, D), e(B * St, 4 * D), et(B * St, D), et(B * St, 4 * D), e(B * St, D)
        T_img = e(B * Si, K2q) if K2q else None
        T_txt = e(B * St, K2a) if K2a else None
        T_o = e(B * Si, K2o) if K2o else None
        T_ao = e(B * St, K2t) if K2t else None
        ya_i, ya_t, yf_i, yf_t = ybuf(B * Si), (None if last else ybuf(B * St)), ybuf(B * Si), (None if last else ybuf(B * St))
        c_img = e(B * Si, 3 * D) if (B > 1 and Si % 256) else None
        c_txt = e(B * St, 3 * D) if (B > 1 and St % 256) else None
        ops.block_sd3_joint_fwd(
            B=B, Si=Si, St=St, H=H, D=D, hd=hd, last=int(last), K2_qkv=K2q, k2r_qkv=kr_q, K2_aqkv=K2a, k2r_aqkv=kr_a, K2_out=K2o, k2r_out=kr_o, K2_aout=K2t, k2r_aout=kr_t,
            scale=env.scale, img=img, txt=txt, mod_img=mod[:, blk.mod_off:], mod_txt=mod[:, blk.mod_off_c:], mod_stride=mod.stride(0),
            w_qkv=blk.qkv.w, b_qkv=blk.qkv.b, w_add_qkv=blk.add_qkv.w, b_add_qkv=blk.add_qkv.b, w_out=blk.to_out.w, b_out=blk.to_out.b,
            w_add_out=None if last else blk.to_add_out.w, b_add_out=None if last else blk.to_add_out.b,
            w_ff1=blk.ff1.w, b_ff1=blk.ff1.b, w_ff2=blk.ff2.w, b_ff2=blk.ff2.b,
            w_ffc1=None if last else blk.ffc1.w, b_ffc1=None if last else blk.ffc1.b, w_ffc2=None if last else blk.ffc2.w, b_ffc2=None if last else blk.ffc2.b,
            A_qkv=A_q, Bb_qkv=Bb_q, A_aqkv=A_a, Bb_aqkv=Bb_a, A_out=A_o, Bb_out=Bb_o, A_aout=A_t, Bb_aout=Bb_t,
            norm_q=blk.norm_q, norm_k=blk.norm_k, norm_added_q=blk.norm_added_q, norm_added_k=blk.norm_added_k, cos=env.cos, sin=env.sin,
            n_img=n_img, n_txt=n_txt, qkv=qkv, Q=Q, K=K, O=O, lse2=lse2, x1_img=x1_img, x1_txt=x1_txt, hpre_img=hpre_img, hpre_txt=hpre_txt,
            T_img=T_img, T_txt=T_txt, T_o=T_o, T_ao=T_ao, ya_img=ya_i, ya_txt=ya_t, yf_img=yf_i, yf_txt=yf_t,
            n2_img=n2_i, n2_txt=n2_t, h_img=h_i, h_txt=h_t, Vt=Vt, c_img=c_img, c_txt=c_txt, out_img=x2_img, out_txt=x2_txt)
        if not save:
            return x2_img, x2_txt, None
        sv = SimpleNamespace(img=img, txt=txt, n_img=n_img, n_txt=n_txt if (T_txt is not None or full) else None, qkv=qkv, Q=Q, K=K, Qt=None, Kt=None, O=O, lse2=lse2,
                             x1_img=x1_img, x1_txt=x1_txt, hpre_img=hpre_img, hpre_txt=hpre_txt, T_img=T_img, T_txt=T_txt, T_o=T_o, T_ao=T_ao, d2=None)
        if full:
            sv.n2_i, sv.n2_t, sv.h_i, sv.h_t, sv.ya_i, sv.ya_t, sv.yf_i, sv.yf_t = n2_i, n2_t, h_i, h_t, ya_i, ya_t, yf_i, yf_t
        return x2_img, x2_txt, sv

    def _block_bwd_c(self, blk, sv, env_li, mod, cos, sin, d_img, d_txt, need_input_grads: bool, dmod=None):
        """the data path of one block's backward through st355_block_sd3_joint_bwd: returns (d_img', d_txt', G) with every intermediate gradient in G — the
        adapter gradients (LoRA) or the weight / bias / modulation gradients (full fine-tune) are taken from them by the caller, the same launches on the same
        operands as the host-side form, after the data path instead of between its steps (independent of it: bit-identical results)"""
        D, H, hd, dev = self.D, self.H, self.hd, self.device_
        B, Si, St, S, Sp = env_li.B, env_li.Si, env_li.St, env_li.S, env_li.Sp
        e = lambda *sh: torch.empty(*sh, dtype=BF16, device=dev)
        last = blk.last
        K2q, kr_q, _, _, At_q, Bbt_q = self._lk(blk.qkv)
        K2a, kr_a, _, _, At_a, Bbt_a = self._lk(blk.add_qkv)
        K2o, kr_o, _, _, At_o, Bbt_o = self._lk(blk.to_out)
        K2t, kr_t, _, _, At_t, Bbt_t = self._lk(None if last else blk.to_add_out)
        G = SimpleNamespace(g_i=e(B * Si, D), dh_i=e(B * Si, 4 * D), dn2_i=e(B * Si, D), dx1_i=e(B * Si, D), dx1g_i=e(B * Si, D),
                            g_t=None, dh_t=None, dn2_t=None, dx1_t=None, dx1g_t=None,
                            dO=(torch.zeros if last else torch.empty)(B * S, D, dtype=BF16, device=dev), dqkv=e(B * S, 3 * D),
                            U_o=e(B * Si, K2o) if K2o else None, U_ao=e(B * St, K2t) if K2t else None, U_q=e(B * Si, K2q) if K2q else None,
                            U_a=e(B * St, K2a) if K2a else None, dn_i=None, dn_t=None, c_img=None, c_txt=None)
        et = (lambda r, c: pad64_empty(r, c, dev)) if dmod is not None else e       # (full fine-tune: the text-stream gradients are weight-gradient operands)
        if not last:
            G.g_t, G.dh_t, G.dn2_t, G.dx1_t, G.dx1g_t = et(B * St, D), et(B * St, 4 * D), e(B * St, D), e(B * St, D), et(B * St, D)
        if B > 1 and Si % 256:
            G.c_img = e(B * Si, 3 * D)
        if B > 1 and St % 256:
            G.c_txt = et(B * St, 3 * D)
        d_img_out = d_txt_out = None
        if need_input_grads:
            G.dn_i, G.dn_t, d_img_out, d_txt_out = e(B * Si, D), e(B * St, D), e(B * Si, D), e(B * St, D)
        dQ, dK = e(B, H, S, hd), e(B, H, S, hd)
        st = {}
        if dmod is not None:
            # full fine-tune: the block's modulation / gate / bias gradients ride in the entry's own passes (csrc/stats.hip) — dmod = the fp32 [B, mod_total] buffer
            st = dict(dmod_img=dmod[:, blk.mod_off:], dmod_txt=dmod[:, blk.mod_off_c:], dmod_stride=dmod.stride(0), ya_img=sv.ya_i, ya_txt=sv.ya_t, yf_img=sv.yf_i,
                      yf_txt=sv.yf_t, gb_ff2=blk.ff2.gb, gb_ff1=blk.ff1.gb, gb_out=blk.to_out.gb, gb_qkv=blk.qkv.gb, gb_add_qkv=blk.add_qkv.gb,
                      gb_ffc2=None if last else blk.ffc2.gb, gb_ffc1=None if last else blk.ffc1.gb, gb_add_out=None if last else blk.to_add_out.gb)
        ops.block_sd3_joint_bwd(**st,
            B=B, Si=Si, St=St, H=H, D=D, hd=hd, last=int(last), need_input_grads=int(need_input_grads),
            K2_qkv=K2q, k2r_qkv=kr_q, K2_aqkv=K2a, k2r_aqkv=kr_a, K2_out=K2o, k2r_out=kr_o, K2_aout=K2t, k2r_aout=kr_t, scale=1.0 / math.sqrt(hd),
            img=sv.img, txt=sv.txt, mod_img=mod[:, blk.mod_off:], mod_txt=mod[:, blk.mod_off_c:], mod_stride=mod.stride(0),
            qkv=sv.qkv, Q=sv.Q, K=sv.K, O=sv.O, lse2=sv.lse2, x1_img=sv.x1_img, x1_txt=sv.x1_txt, hpre_img=sv.hpre_img, hpre_txt=sv.hpre_txt,
            wT_qkv=blk.qkv.wT, wT_add_qkv=blk.add_qkv.wT, wT_out=blk.to_out.wT, wT_add_out=None if last else blk.to_add_out.wT,
            wT_ff1=blk.ff1.wT, wT_ff2=blk.ff2.wT, wT_ffc1=None if last else blk.ffc1.wT, wT_ffc2=None if last else blk.ffc2.wT,
            At_qkv=At_q, Bbt_qkv=Bbt_q, At_aqkv=At_a, Bbt_aqkv=Bbt_a, At_out=At_o, Bbt_out=Bbt_o, At_aout=At_t, Bbt_aout=Bbt_t,
            norm_q=blk.norm_q, norm_k=blk.norm_k, norm_added_q=blk.norm_added_q, norm_added_k=blk.norm_added_k, cos=cos, sin=sin,
            d_img=d_img, d_txt=d_txt, g_img=G.g_i, g_txt=G.g_t, dh_img=G.dh_i, dh_txt=G.dh_t, dn2_img=G.dn2_i, dn2_txt=G.dn2_t, dx1_img=G.dx1_i, dx1g_img=G.dx1g_i,
            dx1_txt=G.dx1_t, dx1g_txt=G.dx1g_t, U_o=G.U_o, U_ao=G.U_ao, dO=G.dO, dqkv=G.dqkv, dQ=dQ, dK=dK, U_qkv=G.U_q, U_aqkv=G.U_a,
            dn_img=G.dn_i, dn_txt=G.dn_t, c_img=G.c_img, c_txt=G.c_txt, d_img_out=d_img_out, d_txt_out=d_txt_out)
        # each stream's rows of dqkv in the operand form the C entry used: in place (a 3-D view, segmented) when B == 1 or tile-aligned, else its compact copy
        G.dq_i = G.c_img if G.c_img is not None else compact(rows_of(G.dqkv, 0, Si, B, S), B, Si)
        G.dq_t = G.c_txt if G.c_txt is not None else compact(rows_of(G.dqkv, Si, St, B, S), B, St)
        return d_img_out, d_txt_out, G

    def _block_bwd(self, ctx, li: int, blk, sv, env, grads):
        """frozen-base LoRA backward of one block (the block_bwd of _walk_blocks_bwd): (d_img, d_txt) with respect to its outputs -> with respect to its inputs,
        and the adapters' gradients.  Block 0 stops at the adapters: the embedders below it are frozen."""
        D, H, hd, dev = self.D, self.H, self.hd, self.device_
        B, St, mod, cos, sin = ctx.B, ctx.St, ctx.mod, ctx.cos, ctx.sin
        Si, S, Sp = env.Si, env.S, env.Sp                # (inside a TREAD route Si is the kept-token count)
        scale = 1.0 / math.sqrt(hd)
        d_img, d_txt = grads
        grads.clear()
        drop = getattr(env, "drop", None)      # LoRA dropout: the masked dA / dx kernels regenerate this forward's masks
        tl = getattr(env, "tl", None)          # T-LoRA: every U = dy B is masked as its T was (the same timesteps: the same mask)
        acc_, gs_ = self.accumulate_lora_grads, self.grad_sync

        def o_rows(lin, lo, rows):
            """this stream's rows of the joint attention output as an adapter-gradient operand: read in place when tile-aligned (image rows), else a compact copy"""
            return None if lin is None or lin.lora is None else compact(rows_of(sv.O, lo, rows, B, S), B, rows)

        if self._c_entry_ok(blk, env, (d_img, d_txt), full=False, backward=True, sv=sv):
            # the data path as ONE C entry point (st355_block_sd3_joint_bwd), then the rank-space adapter gradients from the gradients it left behind
            d_img, d_txt, G = self._block_bwd_c(blk, sv, env, mod, cos, sin, d_img, d_txt, li != 0)
            lora_grads(blk.to_out, o_rows(blk.to_out, 0, Si), sv.T_o, G.dx1g_i, G.U_o, acc_, gs_)
            lora_grads(blk.to_add_out, o_rows(blk.to_add_out, Si, St), sv.T_ao, G.dx1g_t, G.U_ao, acc_, gs_)
            lora_grads(blk.qkv, sv.n_img, sv.T_img, G.dq_i, G.U_q, acc_, gs_)
            lora_grads(blk.add_qkv, sv.n_txt, sv.T_txt, G.dq_t, G.U_a, acc_, gs_)
            return d_img, d_txt
        mi = ctx.mod_i[:, blk.mod_off:blk.mod_off + 6 * D]
        mt = mod[:, blk.mod_off_c:blk.mod_off_c + (2 if blk.last else 6) * D]
        rpb_i = 1 if ctx.rpb_i == 1 else Si
        g_i = ops.scale_cols(d_img, mi[:, 5 * D:6 * D], rpb_i)

        def ff_grads(l1, l2, x1, m6, rpb_, hpre, g_, dh_, T1=None, T2=None, U1=None, U2=None):
            """the adapter gradients of a feed-forward pair (LoKr's and T-LoRA's FeedForward sites): the Linears' inputs are recomputed, nothing is saved for them —
            the modulated LayerNorm rows as the forward made them, the activated rows from the kept pre-activation.  T1 / T2: the forward's masked down projections
            (T-LoRA keeps them: [M, K2] each), U1 / U2: the masked up products of the dx GEMMs above; None for a LoKr group."""
            if l1.lora is not None:
                lora_grads(l1, ops.ln_modulate_fwd(x1, m6[:, 4 * D:5 * D], m6[:, 3 * D:4 * D], rpb_), T1, dh_, U1, acc_, gs_, drop)
            if l2.lora is not None:
                lora_grads(l2, ops.gelu_tanh(hpre), T2, g_, U2, acc_, gs_, drop)

        # (the feed-forward dx GEMMs take the rank-space adapter term as their K-extension: U = dy B masked, then dx += U A in front of the epilogue; nothing for a
        # LoKr group or without an adapter)
        U_f1 = U_f2 = None
        if blk.last:
            U_f2 = lora_up(blk.ff2, g_i, tl=tl)
            dh_i = ops.gemm(g_i, lin_wT(blk.ff2), epilogue=EPI_MUL_GELU_GRAD, aux_in=sv.hpre_img, **lora_dx_kw(blk.ff2, U_f2, drop))
            U_f1 = lora_up(blk.ff1, dh_i, tl=tl)
            dn2_i = ops.gemm(dh_i, lin_wT(blk.ff1), **lora_dx_kw(blk.ff1, U_f1, drop))
            dx1_t = dx1g_t = None
        else:
            g_t = ops.scale_cols(d_txt, mt[:, 5 * D:6 * D], St)
            U_f2, U_c2 = lora_up(blk.ff2, g_i, tl=tl), lora_up(blk.ffc2, g_t, tl=tl)
            dh_i, dh_t = ops.gemm_grouped([dict(a=g_i, w=lin_wT(blk.ff2), epilogue=EPI_MUL_GELU_GRAD, aux_in=sv.hpre_img, **lora_dx_kw(blk.ff2, U_f2, drop)),
                                           dict(a=g_t, w=lin_wT(blk.ffc2), epilogue=EPI_MUL_GELU_GRAD, aux_in=sv.hpre_txt, **lora_dx_kw(blk.ffc2, U_c2, drop))])
            U_f1, U_c1 = lora_up(blk.ff1, dh_i, tl=tl), lora_up(blk.ffc1, dh_t, tl=tl)
            dn2_i, dn2_t = ops.gemm_grouped([dict(a=dh_i, w=lin_wT(blk.ff1), **lora_dx_kw(blk.ff1, U_f1, drop)),
                                             dict(a=dh_t, w=lin_wT(blk.ffc1), **lora_dx_kw(blk.ffc1, U_c1, drop))])
            ff_grads(blk.ffc1, blk.ffc2, sv.x1_txt, mt, St, sv.hpre_txt, g_t, dh_t, getattr(sv, "T_c1", None), getattr(sv, "T_c2", None), U_c1, U_c2)
            del U_c1, U_c2
            dx1_t, dx1g_t = ops.ln_modulate_bwd(dn2_t, sv.x1_txt, mt[:, 4 * D:5 * D], St, dres=d_txt, gate=mt[:, 2 * D:3 * D], want_gated=True)
            del g_t, dh_t, dn2_t
        dn2a = None
        if blk.dual:
            # the MLP's LayerNorm read the stream AFTER the attn2 residual: its gated gradient feeds attn2's output projection, the un-gated one is the
            # gradient of the stream after the joint-attention residual (dx1) — attn2 first, then the joint attention as for a regular block
            d2, mi9 = sv.d2, mod[:, blk.mod_off:blk.mod_off + 9 * D]
            dx1_i, dxg2 = ops.ln_modulate_bwd(dn2_i, sv.x1_img, mi[:, 4 * D:5 * D], Si, dres=d_img, gate=mi9[:, 8 * D:9 * D], want_gated=True)
            U2 = lora_up(blk.to_out2, dxg2, tl=tl)
            dO2 = ops.gemm(dxg2, lin_wT(blk.to_out2), **lora_dx_kw(blk.to_out2, U2, drop))
            lora_dx_finish(blk.to_out2, dO2, U2, drop)
            lora_grads(blk.to_out2, d2.O2, d2.T_o2, dxg2, U2, acc_, gs_, drop)
            dqkv2 = torch.empty(B * Si, 3 * D, dtype=BF16, device=dev)
            dQ2 = torch.empty(B, H, Si, hd, dtype=BF16, device=dev); dK2 = torch.empty_like(dQ2)
            ops.attn_bwd(d2.Q2, d2.K2, d2.Q2t, d2.K2t, d2.qkv2[:, 2 * D:], d2.O2, dO2, d2.lse2b, dQ2, dK2, dqkv2[:, 2 * D:], B, H, Si, d2.Sip, hd, scale)
            ops.qk_norm_rope_bwd(dQ2, dK2, d2.qkv2, blk.norm_q2, blk.norm_k2, cos, sin, dqkv2, B, H, hd, Si, 0, Si)
            Uq2 = lora_up(blk.qkv2, dqkv2, tl=tl)
            if li != 0:
                dn2a = ops.gemm(dqkv2, lin_wT(blk.qkv2), **lora_dx_kw(blk.qkv2, Uq2, drop))
                lora_dx_finish(blk.qkv2, dn2a, Uq2, drop)
            lora_grads(blk.qkv2, d2.n2a, d2.T2, dqkv2, Uq2, acc_, gs_, drop)
            dx1g_i = ops.scale_cols(dx1_i, mi[:, 2 * D:3 * D], Si)
            del dxg2, dO2, dQ2, dK2, dqkv2, U2, Uq2, d2
        else:
            dx1_i, dx1g_i = ops.ln_modulate_bwd(dn2_i, sv.x1_img, mi[:, 4 * D:5 * D], rpb_i, dres=d_img, gate=mi[:, 2 * D:3 * D], want_gated=True)
        ff_grads(blk.ff1, blk.ff2, sv.x1_img, mi, rpb_i, sv.hpre_img, g_i, dh_i, getattr(sv, "T_f1", None), getattr(sv, "T_f2", None), U_f1, U_f2)
        del g_i, dh_i, dn2_i, U_f1, U_f2
        # attention output projections -> dO rows of both streams (+ adapter grads); a context_pre_only block has no txt rows (and no to_add_out)
        dO = (torch.zeros if blk.last else torch.empty)(B * S, D, dtype=BF16, device=dev)
        dO_i, dO_t = rows_of(dO, 0, Si, B, S), rows_of(dO, Si, St, B, S)
        U_i, U_t = lora_up(blk.to_out, dx1g_i, tl=tl), lora_up(blk.to_add_out, dx1g_t, tl=tl)
        after = []
        probs = _stream_problems(B, S, Si, dict(a=dx1g_i, w=lin_wT(blk.to_out), out=dO_i, **lora_dx_kw(blk.to_out, U_i, drop)), after)
        if not blk.last:
            probs += _stream_problems(B, S, St, dict(a=dx1g_t, w=lin_wT(blk.to_add_out), out=dO_t, **lora_dx_kw(blk.to_add_out, U_t, drop)), after)
        ops.gemm_grouped(probs)
        for f in after:
            f()
        lora_dx_finish(blk.to_out, dO_i, U_i, drop)               # the adapter term of dO, masked, before the attention backward reads it (the joint buffer's rows in place)
        lora_dx_finish(blk.to_add_out, dO_t, U_t, drop)
        lora_grads(blk.to_out, o_rows(blk.to_out, 0, Si), sv.T_o, dx1g_i, U_i, acc_, gs_, drop)
        lora_grads(blk.to_add_out, o_rows(blk.to_add_out, Si, St), sv.T_ao, dx1g_t, U_t, acc_, gs_, drop)
        del dx1g_i, dx1g_t, U_i, U_t, dO_i, dO_t
        dqkv = torch.empty(B * S, 3 * D, dtype=BF16, device=dev)
        dQ = torch.empty(B, H, S, hd, dtype=BF16, device=dev); dK = torch.empty_like(dQ)
        ops.attn_bwd(sv.Q, sv.K, sv.Qt, sv.Kt, sv.qkv[:, 2 * D:], sv.O, dO, sv.lse2, dQ, dK, dqkv[:, 2 * D:], B, H, S, Sp, hd, scale)
        ops.qk_norm_rope_bwd(dQ, dK, sv.qkv, blk.norm_q, blk.norm_k, cos, sin, dqkv, B, H, hd, Si, 0, S)
        ops.qk_norm_rope_bwd(dQ, dK, sv.qkv, blk.norm_added_q, blk.norm_added_k, cos, sin, dqkv, B, H, hd, St, Si, S)
        del dQ, dK, dO
        # the two streams' rows of the joint dqkv: the image rows in place (segmented operands), the 154 text rows as a compact copy
        sites = [(blk.qkv, compact(rows_of(dqkv, 0, Si, B, S), B, Si), sv.n_img, sv.T_img, Si),
                 (blk.add_qkv, compact(rows_of(dqkv, Si, St, B, S), B, St), sv.n_txt, sv.T_txt, St)]
        Us = [lora_up(lin, dq, tl=tl) for (lin, dq, _, _, _) in sites]
        if li != 0:               # (block 0: frozen embedders below, only the adapter gradients remain)
            dns = [torch.empty(B * rows, D, dtype=BF16, device=dev) for (_, _, _, _, rows) in sites]
            ops.gemm_grouped([dict(a=dq, w=lin_wT(lin), out=dn_, **lora_dx_kw(lin, U, drop)) for (lin, dq, _, _, _), U, dn_ in zip(sites, Us, dns)])
            for (lin, _, _, _, _), U, dn_ in zip(sites, Us, dns):      # the adapter term of the norm inputs' gradients, masked, before the norm backward reads them
                lora_dx_finish(lin, dn_, U, drop)
        for (lin, dq, n_in, T_, _), U in zip(sites, Us):
            lora_grads(lin, n_in, T_, dq, U, acc_, gs_, drop)
        if li != 0:
            d_img, _ = ops.ln_modulate_bwd(dns[0], sv.img, mi[:, D:2 * D], rpb_i, dres=dx1_i)
            if dn2a is not None:             # the second reader of LN(img): attn2's modulated input (scale_msa2)
                d_img, _ = ops.ln_modulate_bwd(dn2a, sv.img, mod[:, blk.mod_off + 7 * D:blk.mod_off + 8 * D], Si, dres=d_img)
            d_txt, _ = ops.ln_modulate_bwd(dns[1], sv.txt, mt[:, :D] if blk.last else mt[:, D:2 * D], St, dres=dx1_t)
        return d_img, d_txt

    def _block_bwd_full(self, ctx, fb, blk, sv, env, grads):
        """full fine-tune backward of one block (the block_bwd of _walk_blocks_bwd): (d_img, d_txt) with respect to its outputs -> with respect to its inputs, and
        every weight / bias / modulation gradient of the block (fb: the backward's FullGrads)"""
        D, H, hd, dev = self.D, self.H, self.hd, self.device_
        B, St, mod, cos, sin = ctx.B, ctx.St, ctx.mod, ctx.cos, ctx.sin
        Si, S, Sp = env.Si, env.S, env.Sp                # (inside a TREAD route Si is the kept-token count)
        scale = 1.0 / math.sqrt(hd)
        dmod, wgrad = fb.dmod, fb.wgrad
        d_img, d_txt = grads
        grads.clear()

        def qk_bwd(dQ_, dK_, qkv_, wq, wk, dqkv_, rows, pos0, S_, gq, gk):
            """RMSNorm (+ identity RoPE) backward of one stream's q / k; with norm weights (SD3.5) also their gradients (sd3/transformer.py:155-165)"""
            if wq is None and wk is None:
                ops.qk_norm_rope_bwd(dQ_, dK_, qkv_, wq, wk, cos, sin, dqkv_, B, H, hd, rows, pos0, S_)
            else:
                ops.qk_norm_rope_bwd_wgrad(dQ_, dK_, qkv_, wq, wk, cos, sin, dqkv_, B, H, hd, rows, pos0, S_, gq, gk)

        def grad_rows(t, lo, n, seg: bool = False):
            """rows [lo, lo+n) of every batch element of a joint [B*S, C] buffer as a weight-gradient operand.  seg: in place — a [B, n, C] strided view, the
            segmented-contraction form of st355_gemm_tn_seg_bf16 — when n is a whole number of 64-row K-tiles (the image rows of every bucket); else (the text
            rows, and callers that also read the operand as a plain matrix) a compact copy, its row count zero-tailed to 64 (pad64 takes it as is)"""
            if B == 1:
                return t[lo:lo + n]
            v = t.view(B, S, -1)[:, lo:lo + n]
            if seg and n % 64 == 0 and n >= 128:
                return v
            o = pad64_empty(B * n, t.shape[1], dev)
            o.view(B, n, -1).copy_(v)
            return o

        if self._c_entry_ok(blk, env, (d_img, d_txt), full=True, backward=True, sv=sv):
            # the data path as ONE C entry point (st355_block_sd3_joint_bwd).  Every bias / modulation-shift / -scale / gate gradient of the block is written by the
            # entry itself — the column sums ride in its scale_cols and LayerNorm-backward passes, csrc/stats.hip; only the weight gradients are left, taken from
            # the gradients it kept
            d_img, d_txt, G = self._block_bwd_c(blk, sv, env, mod, cos, sin, d_img, d_txt, True, dmod=dmod)
            wgrad(blk.ff2, G.g_i, sv.h_i, bias=False)
            wgrad(blk.ff1, G.dh_i, sv.n2_i, bias=False)
            if not blk.last:
                wgrad(blk.ffc2, G.g_t, sv.h_t, bias=False)
                wgrad(blk.ffc1, G.dh_t, sv.n2_t, bias=False)
            wgrad(blk.to_out, G.dx1g_i, grad_rows(sv.O, 0, Si, seg=True), bias=False)
            if not blk.last:
                wgrad(blk.to_add_out, G.dx1g_t, grad_rows(sv.O, Si, St), bias=False)
            wgrad(blk.qkv, G.c_img if G.c_img is not None else grad_rows(G.dqkv, 0, Si, seg=True), sv.n_img, bias=False)       # (c_*: the compact copy the entry left)
            wgrad(blk.add_qkv, G.c_txt if G.c_txt is not None else grad_rows(G.dqkv, Si, St), sv.n_txt, bias=False)
            return d_img, d_txt
        mi = mod[:, blk.mod_off:blk.mod_off + 6 * D]; dmi = dmod[:, blk.mod_off:blk.mod_off + 6 * D]
        nct = 2 if blk.last else 6
        mt = mod[:, blk.mod_off_c:blk.mod_off_c + nct * D]; dmt = dmod[:, blk.mod_off_c:blk.mod_off_c + nct * D]
        # ---- MLP branch (host-sequenced form: SD3.5 dual-attention blocks, trainable q / k norms, ST355_BLOCK_ABI=0).  Every modulation / gate / bias
        # gradient rides in the pass that streams its operands — the same fused entry points the C block sequences (csrc/stats.hip) ----
        g_i = ops.scale_cols_stats(d_img, mi[:, 5 * D:6 * D], Si, y_branch=sv.yf_i, d_gate=dmi[:, 5 * D:6 * D], d_bias=blk.ff2.gb)     # + d gate_mlp, d b_ff2
        wgrad(blk.ff2, g_i, sv.h_i, bias=False)
        dh_i = ops.gemm(g_i, blk.ff2.wT, epilogue=EPI_MUL_GELU_GRAD, aux_in=sv.hpre_img)
        wgrad(blk.ff1, dh_i, sv.n2_i, bias=False)
        dn2_i = ops.gemm(dh_i, blk.ff1.wT)
        dn2a = None
        if blk.dual:
            d2 = sv.d2
            mi9 = mod[:, blk.mod_off:blk.mod_off + 9 * D]; dmi9 = dmod[:, blk.mod_off:blk.mod_off + 9 * D]
            # + d shift_mlp, d scale_mlp, d gate_msa2 = sum d x1 * y_attn2, d b_to_out2 = sum gate_msa2 * d x1
            dx1_i, dxg2 = ops.ln_modulate_bwd_stats(dn2_i, sv.x1_img, mi[:, 4 * D:5 * D], Si, dmi[:, 3 * D:4 * D], dmi[:, 4 * D:5 * D], dres=d_img,
                                                    gate=mi9[:, 8 * D:9 * D], y_branch=d2.ya2, d_gate=dmi9[:, 8 * D:9 * D], d_bias=blk.to_out2.gb, want_gated=True)
            ops.colsum_rows(dh_i, Si, Si, B, blk.ff1.gb)
            wgrad(blk.to_out2, dxg2, d2.O2, bias=False)
            dO2 = ops.gemm(dxg2, blk.to_out2.wT)
            dqkv2 = torch.empty(B * Si, 3 * D, dtype=BF16, device=dev)
            dQ2 = torch.empty(B, H, Si, hd, dtype=BF16, device=dev); dK2 = torch.empty_like(dQ2)
            ops.attn_bwd(d2.Q2, d2.K2, d2.Q2t, d2.K2t, d2.qkv2[:, 2 * D:], d2.O2, dO2, d2.lse2b, dQ2, dK2, dqkv2[:, 2 * D:], B, H, Si, d2.Sip, hd, scale)
            qk_bwd(dQ2, dK2, d2.qkv2, blk.norm_q2, blk.norm_k2, dqkv2, Si, 0, Si, blk.g_norm_q2, blk.g_norm_k2)
            wgrad(blk.qkv2, dqkv2, d2.n2a)
            dn2a = ops.gemm(dqkv2, blk.qkv2.wT)
            dx1g_i = ops.scale_cols_stats(dx1_i, mi[:, 2 * D:3 * D], Si, y_branch=sv.ya_i, d_gate=dmi[:, 2 * D:3 * D], d_bias=blk.to_out.gb)   # + d gate_msa, d b_to_out
            del dxg2, dO2, dQ2, dK2, dqkv2, d2
        else:
            # + d shift_mlp, d scale_mlp, d gate_msa = sum d x1 * y_attn, d b_to_out = sum gate_msa * d x1
            dx1_i, dx1g_i = ops.ln_modulate_bwd_stats(dn2_i, sv.x1_img, mi[:, 4 * D:5 * D], Si, dmi[:, 3 * D:4 * D], dmi[:, 4 * D:5 * D], dres=d_img,
                                                      gate=mi[:, 2 * D:3 * D], y_branch=sv.ya_i, d_gate=dmi[:, 2 * D:3 * D], d_bias=blk.to_out.gb, want_gated=True)
            ops.colsum_rows(dh_i, Si, Si, B, blk.ff1.gb)
        del g_i, dh_i, dn2_i
        dx1_t = dx1g_t = None
        if not blk.last:
            g_t = ops.scale_cols_stats(d_txt, mt[:, 5 * D:6 * D], St, y_branch=sv.yf_t, d_gate=dmt[:, 5 * D:6 * D], d_bias=blk.ffc2.gb)
            wgrad(blk.ffc2, g_t, sv.h_t, bias=False)
            dh_t = ops.gemm(g_t, blk.ffc2.wT, epilogue=EPI_MUL_GELU_GRAD, aux_in=sv.hpre_txt)
            wgrad(blk.ffc1, dh_t, sv.n2_t, bias=False)
            dn2_t = ops.gemm(dh_t, blk.ffc1.wT)
            dx1_t, dx1g_t = ops.ln_modulate_bwd_stats(dn2_t, sv.x1_txt, mt[:, 4 * D:5 * D], St, dmt[:, 3 * D:4 * D], dmt[:, 4 * D:5 * D], dres=d_txt,
                                                      gate=mt[:, 2 * D:3 * D], y_branch=sv.ya_t, d_gate=dmt[:, 2 * D:3 * D], d_bias=blk.to_add_out.gb, want_gated=True)
            ops.colsum_rows(dh_t, St, St, B, blk.ffc1.gb)
            del g_t, dh_t, dn2_t
        # ---- attention output projections ----
        O_i = grad_rows(sv.O, 0, Si)
        wgrad(blk.to_out, dx1g_i, O_i, bias=False)
        dO = (torch.zeros if blk.last else torch.empty)(B * S, D, dtype=BF16, device=dev)
        after = []
        probs = _stream_problems(B, S, Si, dict(a=dx1g_i, w=blk.to_out.wT, out=rows_of(dO, 0, Si, B, S)), after)
        if not blk.last:
            probs += _stream_problems(B, S, St, dict(a=dx1g_t, w=blk.to_add_out.wT, out=rows_of(dO, Si, St, B, S)), after)
        ops.gemm_grouped(probs)
        for f in after:
            f()
        if not blk.last:
            wgrad(blk.to_add_out, dx1g_t, grad_rows(sv.O, Si, St), bias=False)
        del dx1g_i, dx1g_t, O_i
        # ---- attention ----
        dqkv = torch.empty(B * S, 3 * D, dtype=BF16, device=dev)
        dQ = torch.empty(B, H, S, hd, dtype=BF16, device=dev); dK = torch.empty_like(dQ)
        ops.attn_bwd(sv.Q, sv.K, sv.Qt, sv.Kt, sv.qkv[:, 2 * D:], sv.O, dO, sv.lse2, dQ, dK, dqkv[:, 2 * D:], B, H, S, Sp, hd, scale)
        qk_bwd(dQ, dK, sv.qkv, blk.norm_q, blk.norm_k, dqkv, Si, 0, S, blk.g_norm_q, blk.g_norm_k)
        qk_bwd(dQ, dK, sv.qkv, blk.norm_added_q, blk.norm_added_k, dqkv, St, Si, S, blk.g_norm_added_q, blk.g_norm_added_k)
        del dQ, dK, dO
        ops.colsum_rows(dqkv, Si, S, B, blk.qkv.gb)                    # d b_qkv / d b_add_qkv: each stream's rows of the joint dqkv, summed in place
        ops.colsum_rows(dqkv[Si:], St, S, B, blk.add_qkv.gb)
        dq_i, dq_t = grad_rows(dqkv, 0, Si), grad_rows(dqkv, Si, St)
        wgrad(blk.qkv, dq_i, sv.n_img, bias=False)
        wgrad(blk.add_qkv, dq_t, sv.n_txt, bias=False)
        dn_i, dn_t = ops.gemm_grouped([dict(a=dq_i, w=blk.qkv.wT), dict(a=dq_t, w=blk.add_qkv.wT)])
        d_img, _ = ops.ln_modulate_bwd_stats(dn_i, sv.img, mi[:, D:2 * D], Si, dmi[:, :D], dmi[:, D:2 * D], dres=dx1_i)      # + d shift_msa, d scale_msa
        if dn2a is not None:                  # the second reader of LN(img): attn2's modulated input (shift_msa2, scale_msa2)
            d_img, _ = ops.ln_modulate_bwd_stats(dn2a, sv.img, mod[:, blk.mod_off + 7 * D:blk.mod_off + 8 * D], Si, dmi9[:, 6 * D:7 * D], dmi9[:, 7 * D:8 * D],
                                                 dres=d_img)
        if blk.last:                          # AdaLayerNormContinuous: chunks (scale, shift)
            d_txt, _ = ops.ln_modulate_bwd_stats(dn_t, sv.txt, mt[:, :D], St, dmt[:, D:2 * D], dmt[:, :D], dres=None)
        else:
            d_txt, _ = ops.ln_modulate_bwd_stats(dn_t, sv.txt, mt[:, D:2 * D], St, dmt[:, :D], dmt[:, D:2 * D], dres=dx1_t)
        return d_img, d_txt

    def _engine_forward(self, latents, enc, pooled, timestep, save: bool, full: bool = False, want_ig: bool = False, capture: Optional[int] = None):
        D, H, hd = self.D, self.H, self.hd
        B, C, Hh, Ww = latents.shape
        h, w = Hh // 2, Ww // 2
        Si, St = h * w, enc.shape[1]
        S = Si + St
        Sp = (S + 63) // 64 * 64
        dev = self.device_
        if self.lora_tlora is not None:     # T-LoRA: the adapter scale of this forward is multiplier (alpha / r), in eval() forwards times the validation strength
            mult = self.tlora_multiplier * (1.0 if self.training else self.lokr_validation_strength)
            for g in self.lora_groups:
                g.scale = mult * g.tlora_scale
        for g in self.lora_groups:
            g.pack()
            if g.dora is not None:          # DoRA: the row scale of the current A / B / m folded into W and B_blk, once per forward
                g.fold()
        if self.lora_lokr:                  # LoKr: W + s kron(w1, w2) of the current factors, once per forward (eval() forwards: times the validation strength)
            mult = self.lokr_multiplier * (1.0 if self.training else self.lokr_validation_strength)
            for g in self.lora_groups:
                g.fold(mult)
        pos, cos, sin = self._tables(h, w, S, B)
        # ---- embeddings (sd3/transformer.py:623-700) ----
        patches = ops.patchify(latents, order=0).view(B * Si, 4 * C)
        img = ops.gemm(patches, self.l_patch.w, bias=self.l_patch.b, epilogue=EPI_ADD, aux_in=pos)
        enc2d = enc.reshape(B * St, -1).contiguous()
        txt = ops.gemm(enc2d, self.l_ctx.w, bias=self.l_ctx.b)
        tokenwise = timestep.dim() == 2
        if tokenwise and tuple(timestep.shape) != (B, Si):
            raise ValueError(f"SD3 tokenwise timesteps expected sequence length {Si}, got {timestep.shape[1]}.")      # sd3/transformer.py:625-626
        t32 = timestep.to(device=dev, dtype=F32).reshape(-1).contiguous()
        tproj = ops.timestep_proj(t32, 256, 1.0)
        t1 = ops.gemm(tproj, self.l_t1.w, bias=self.l_t1.b); st1 = ops.silu(t1)
        pooled_b = pooled.to(BF16).contiguous()
        p1 = ops.gemm(pooled_b, self.l_p1.w, bias=self.l_p1.b); sp1 = ops.silu(p1)
        mod_i, rpb_i = None, Si
        if tokenwise:
            # TOKENWISE timesteps [B, S_img] (CREPA self-flow; sd3/transformer.py:61-75, 126-142, 680-685, 876): one conditioning row per image token — the image
            # stream's shift / scale / gate rows and norm_out's (scale, shift) are per TOKEN (the AdaLN / gated-residual kernels index their modulation row by
            # row // rows_per_batch: rows_per_batch = 1), the context stream is conditioned on the mean over the tokens.  The per-token modulation rows of every
            # block are ONE GEMM [B * S_img, D] x [mod_total, D]^T (B * S_img * mod_total bf16: 14 GB for SD3-Medium at 1024^2, batch 8 — HBM holds it).
            if full:
                raise NotImplementedError("tokenwise timesteps under a full fine-tune (per-token modulation gradients) are not implemented on the st355 path")
            if any(b.dual for b in self.blocks):
                raise NotImplementedError("tokenwise timesteps with SD3.5 dual-attention blocks: the reference chunks SD35AdaLayerNormZeroX's [B, S, 9D] output along the "
                                          "token axis (sd3/transformer.py:155-164) — not a defined computation")
            pe = ops.gemm(sp1, self.l_p2.w, bias=self.l_p2.b)                                         # [B, D]: the pooled-text embedding, shared by a sample's tokens
            temb_tok = ops.gemm(st1, self.l_t2.w, bias=self.l_t2.b, epilogue=EPI_ADD, aux_in=pe[:, None, :].expand(B, Si, D).reshape(B * Si, D))
            tsum = torch.empty(B, D, dtype=F32, device=dev)
            ops.colsum_prod(temb_tok, tsum, rows_per_batch=Si)
            temb = (tsum / Si).to(BF16)                                                               # temb_context = temb.mean(dim=1)   (:681-682)
            mod_i = ops.gemm(ops.silu(temb_tok), self.mod_w, bias=self.mod_b)                         # [B * S_img, mod_total]
            rpb_i = 1
        else:
            temb = ops.add(ops.gemm(st1, self.l_t2.w, bias=self.l_t2.b), ops.gemm(sp1, self.l_p2.w, bias=self.l_p2.b))
        st = ops.silu(temb)
        mod = ops.gemm(st, self.mod_w, bias=self.mod_b)
        if mod_i is None:
            mod_i = mod
        ctx = SimpleNamespace(B=B, Si=Si, St=St, S=S, Sp=Sp, cos=cos, sin=sin, mod=mod, mod_i=mod_i, rpb_i=rpb_i, blocks=[], C=C, Hh=Hh, Ww=Ww)
        if full and save:
            ctx.emb = SimpleNamespace(patches=patches, enc2d=enc2d, tproj=tproj, t1=t1, st1=st1, pooled=pooled_b, p1=p1, sp1=sp1, temb=temb, st=st)
        scale = 1.0 / math.sqrt(hd)
        # LoRA dropout: training forwards only (validation sampling and eval() forwards are the p = 0 computation).  The call counter advances here, once per
        # training forward — the blocks below, their recompute passes and the backward all read the value it advanced to
        drop = self.lora_dropout if (save and self.training and not full and self.lora_groups) else None
        if drop is not None:
            drop.advance()
        # T-LoRA: the [B] timesteps stay on the device — as the component received them when the mask kernel reads that dtype, else their fp32 image (exact for
        # every integer step) — bound to the rank table for this forward, its recompute passes and its backward; every forward of the component, eval() included
        tl = None
        if self.lora_tlora is not None and self.lora_groups and not full:
            if tokenwise:
                raise NotImplementedError("lycoris tlora with tokenwise timesteps: the active rank is a function of ONE timestep per sample (the reference's int(t) over "
                                          "a [B, S] list fails too); not built on the st355 path")
            direct = timestep.device == dev and timestep.dtype in (F32, BF16, torch.int64) and timestep.is_contiguous()
            tl = self.lora_tlora.at(timestep.reshape(-1) if direct else t32)
        env = SimpleNamespace(B=B, Si=Si, St=St, S=S, Sp=Sp, cos=cos, sin=sin, mod=mod, mod_i=mod_i, rpb_i=rpb_i, scale=scale, full=full, drop=drop, tl=tl)
        ctx.env, ctx.blocks, ctx.ck = env, [None] * len(self.blocks), {}
        # activation-checkpoint plan (sd3/transformer.py:716-833; training/checkpoint_plan.py): a checkpointed segment keeps only its input
        from ..training.checkpoint_plan import segments as _segments
        ctx.segs = _segments(len(self.blocks), bool(save and self.gradient_checkpointing), self.gradient_checkpointing_interval,
                             self.gradient_checkpointing_segment_stride)
        # TREAD routing (sd3/transformer.py:694-706, 796-803; training/tread.py): only while training, between the route's two blocks the IMAGE stream is a
        # per-sample subset of its tokens.  Under routing the reference drops the segmented checkpoint form for the per-block one (:716-728)
        from ..training.tread import normalise_routes
        routes = normalise_routes(self._tread_routes, len(self.blocks)) if (save and self.training and self._tread_router is not None) else []
        if routes and tokenwise:
            raise NotImplementedError("tokenwise timesteps under TREAD routing (the routed tokens' modulation rows would be gathered too) are not implemented")
        if routes:
            from ..training.checkpoint_plan import per_block as _per_block
            ctx.segs = _per_block(len(self.blocks), bool(self.gradient_checkpointing), self.gradient_checkpointing_interval, self.gradient_checkpointing_segment_stride)
        ctx.envs, ctx.route_start, ctx.route_end = [env] * len(self.blocks), {}, {}
        ctx.taps = self._make_taps(save, want_ig, tokenwise, capture)
        rp, info, saved, env_cur = 0, None, None, env
        last = capture if capture is not None else len(self.blocks) - 1          # a capture forward (Self-Flow's teacher) ends behind the captured block
        for (s0, n, ck) in ctx.segs:
            for bi in range(s0, min(s0 + n, last + 1)):
                if rp < len(routes) and info is None and bi == routes[rp]["start_layer_idx"]:
                    info = self._tread_router.get_mask(img.view(B, Si, D), mask_ratio=routes[rp]["selection_ratio"], force_keep=getattr(self, "_force_keep_mask", None))
                    saved = img
                    img = ops.gather_rows(img.view(B, Si, D), info.keep_i32()).view(-1, D)          # TREADRouter.start_route
                    K = info.ids_keep.shape[1]
                    env_cur = SimpleNamespace(**{**vars(env), "Si": K, "S": K + St, "Sp": (K + St + 63) // 64 * 64})
                    ctx.route_start[bi] = info
                if ck and bi == s0:
                    ctx.ck[s0] = (img, txt)
                ctx.envs[bi] = env_cur
                img, txt, ctx.blocks[bi] = self._block_fwd(self.blocks[bi], img, txt, env_cur, save and not ck)
                for tap in ctx.taps:                          # each on this block's image-stream output (the recompute pass, _recompute_segment, never taps)
                    tap.tap(bi, img.view(B, Si, D))
                if info is not None and bi == routes[rp]["end_layer_idx"]:
                    full_seq = saved.clone()                                                        # TREADRouter.end_route(original_x=saved)
                    ops.scatter_rows(img.view(B, env_cur.Si, D), info.keep_i32(), full_seq.view(B, Si, D))
                    img, ctx.route_end[bi] = full_seq, info
                    info, saved, env_cur, rp = None, None, env, rp + 1
        if info is not None:
            raise ValueError("TREAD route does not end inside the block stack (end_layer_idx)")
        if capture is not None:
            for tap in ctx.taps:
                tap.finish(Hh, Ww)
            return None, ctx
        # ---- output head: AdaLayerNormContinuous (scale, shift), proj_out, unpatchify "nhwpqc->nchpwq" ----
        mo = mod_i[:, self.mod_off_out:self.mod_off_out + 2 * D]
        n_out = ops.ln_modulate_fwd(img, mo[:, :D], mo[:, D:2 * D], rpb_i)
        out = ops.gemm(n_out, self.l_out.w, bias=self.l_out.b)
        if save:
            ctx.x_img_final = img
            if full:
                ctx.n_out = n_out
        for tap in ctx.taps:
            tap.finish(Hh, Ww)
        return ops.unpatchify(out.view(B, Si, -1), self.out_channels, Hh, Ww, order=1), ctx

    def _make_taps(self, save: bool, want_ig: bool, tokenwise: bool, capture: Optional[int] = None) -> list:
        """the per-forward taps of the configured regularisers, in their launch order: LayerSync, Internal Guidance, NextLat (engine.py: `tap` after every block of
        the saving forward, `finish` after the output head, `backward` right before the backward of block `tap.block`; `key` names the extra output)"""
        taps, routed = [], self._tread_router is not None
        if capture is not None:                    # Self-Flow's teacher forward: no-grad, nothing kept, one block's image rows copied out
            if save or not 0 <= int(capture) < len(self.blocks):
                raise ValueError(f"crepa_capture_block_index must name a block in [0, {len(self.blocks) - 1}] of a no-grad forward, got {capture}")
            return [CaptureTap(int(capture))]
        if save and self._layersync is not None:
            if routed:
                raise NotImplementedError("LayerSync under TREAD routing (the student and the teacher block would see different token subsets) is not built on the st355 path")
            if tokenwise:
                raise NotImplementedError("LayerSync with tokenwise timesteps is not built on the st355 path")
            taps.append(LayerSyncTap(*self._layersync))
        if self._ig_block is not None and (save or want_ig):
            if save and routed:
                raise NotImplementedError("Internal Guidance under TREAD routing (the routed block's token count no longer matches the diffusion target) is not built on the st355 path")
            taps.append(InternalGuidanceTap(self._ig_head(), self.out_channels))
        elif want_ig:
            raise ValueError("The transformer does not have an internal_guidance_head.")          # internal_guidance.py:405
        if self._nl_block is not None and save:
            if routed:
                raise NotImplementedError("NextLat under TREAD routing (the routed block's token rows are no longer neighbours in the sequence) is not built on the st355 path")
            taps.append(NextLatTap(self._nl_head(), self._nl_mode))
        if self._sf_block is not None and save:
            if routed:
                raise NotImplementedError("crepa_enabled (self_flow) under TREAD routing (the student's routed block and the teacher's would see different token subsets) is "
                                          "not built on the st355 path")
            if self._sf is None:
                raise RuntimeError("Self-Flow: no projector is laid out for training (add_lora_adapter() after set_self_flow())")
            self._sf_tap = SelfFlowTap(self._sf, self._sf_feats)
            self._sf_feats = None
            taps.append(self._sf_tap)
        if self._st_cfg is not None and save:
            c = self._st_cfg
            if routed:
                raise NotImplementedError("distillation_method=self_transcendence under TREAD routing (the routed block's token count no longer matches the target's) is "
                                          "not built on the st355 path")
            if tokenwise:
                raise NotImplementedError("distillation_method=self_transcendence with tokenwise timesteps is not built on the st355 path")
            if self._st is None:
                raise RuntimeError("Self-Transcendence: no projector is laid out for training (add_lora_adapter() after set_self_transcendence())")
            target, sigmas = self._st_in or (None, None)
            self._st_in = None
            taps.append(SelfTranscendenceTap(self._st, c.stage, target, sigmas, c.timestep_min, c.timestep_max, c.cfg_scale, off=c.off))
        return taps

    def set_self_transcendence(self, stage: str, student_block, teacher_block=None, hidden_dim: int = 2048, timestep_min: float = 0.4, timestep_max: float = 0.7,
                               cfg_scale: float = 30.0):
        """Self-Transcendence (helpers/distillation/self_transcendence/distiller.py; the reference reads `layer_{i}` of the hidden-state buffer filled at
        sd3/transformer.py:872): the 0-based joint block whose image-stream output feeds the projector Linear(D -> hidden_dim) -> SiLU -> Linear -> SiLU ->
        Linear(hidden_dim -> D), and — stage `self` — the block of the frozen teacher's forward it is trained to.  Call it before `add_lora_adapter` (the projector's
        fp32 masters go to the tail of the adapter arena).  A training forward then takes `self_transcendence_target` (stage `vae`: the diffusion target
        [B, C, H, W]; stage `self`: what a no-grad forward at batch 2B — conditional rows, then unconditional — with `crepa_capture_block_index=teacher_block` inside
        `teacher_values(snapshot)` returned as `crepa_hidden_states`) and `self_transcendence_sigmas` [B], and also returns the masked per-sample MSE
        `self_transcendence_guide_loss`; the backward takes its gradient at the student block.  `self_transcendence_off(True)`: the weight is 0 from here on —
        the tap launches nothing.  LoRA only."""
        if stage not in ("vae", "self"):
            raise ValueError("Self-Transcendence stage must be either 'vae' or 'self'.")
        s_, t_ = self_transcendence_indices(student_block, teacher_block, len(self.blocks))
        if stage == "self" and t_ is None:
            raise ValueError("Self-Transcendence self stage requires teacher_block.")
        if self._ig_block is not None or self._nl_block is not None or self._sf_block is not None or self._layersync is not None:
            raise NotImplementedError("distillation_method=self_transcendence together with LayerSync / Internal Guidance / NextLat / Self-Flow is not built on the st355 "
                                      "path (they claim the same arena tail)")
        if self.full:
            raise NotImplementedError("distillation_method=self_transcendence under a full fine-tune is not built on the st355 path (built: SD3 LoRA)")
        cfg = SimpleNamespace(stage=stage, student_block=s_, teacher_block=t_, hidden_dim=int(hidden_dim), timestep_min=float(timestep_min),
                              timestep_max=float(timestep_max), cfg_scale=float(cfg_scale), off=False)
        if self._st is not None:
            if cfg.hidden_dim != self._st.Hp:
                raise RuntimeError(f"set_self_transcendence: the projector is laid out with projector_hidden_dim={self._st.Hp}, not {cfg.hidden_dim}")
            self._st_cfg, self._st.block = cfg, s_          # the projector exists: only the tap and its settings move
            return
        if self.lora_groups:
            raise RuntimeError("set_self_transcendence: the trainable arena is already laid out without the projector — call it before add_lora_adapter()")
        self._st_cfg = cfg

    def self_transcendence_off(self, off: bool = True):
        """stop_step reached: the guide loss takes no part from here on — the tap launches nothing, returns a constant 0 and zeroes the projector's gradient views"""
        self._st_cfg.off = bool(off)

    def set_self_flow(self, student_block, teacher_block):
        """Self-Flow (CREPA with crepa_feature_source=self_flow; the reference captures `layer_{i}` at sd3/transformer.py:872): the 0-based joint block whose
        image-stream output feeds the projector LayerNorm -> Linear(D -> D), and the block of the EMA teacher's forward it is aligned to.  Call it before
        `add_lora_adapter` (the projector's fp32 masters go to the tail of the adapter arena).  A training forward then takes `crepa_teacher_features` — what a no-grad
        forward with `crepa_capture_block_index=teacher_block` inside `teacher_values(shadow)` returned as `crepa_hidden_states` — and also returns the mean cosine
        `crepa_similarity`; the backward takes its gradient at the student block.  LoRA only: a full fine-tune refuses tokenwise timesteps."""
        s_, t_ = self_flow_indices(student_block, teacher_block, len(self.blocks))
        if self._st_cfg is not None:
            raise NotImplementedError("distillation_method=self_transcendence together with Self-Flow is not built on the st355 path (both claim the tail of the arena that trains)")
        if self._ig_block is not None or self._nl_block is not None or self._layersync is not None:
            raise NotImplementedError("crepa_enabled (self_flow) together with LayerSync / Internal Guidance / NextLat is not built on the st355 path (they refuse tokenwise "
                                      "timesteps or claim the same arena tail)")
        if self.full or any(b.dual for b in self.blocks):
            raise NotImplementedError("crepa_enabled (self_flow) needs tokenwise timesteps, which a full fine-tune and the SD3.5 dual-attention blocks refuse on the st355 path")
        if self._sf is not None:
            self._sf_block, self._sf_teacher_block = s_, t_           # the projector exists: only the taps move
            self._sf.block, self._sf.teacher_block = s_, t_
            return
        if self.lora_groups:
            raise RuntimeError("set_self_flow: the trainable arena is already laid out without the projector — call it before add_lora_adapter()")
        self._sf_block, self._sf_teacher_block = s_, t_

    def self_flow_cutoff(self):
        """the scheduler's weight of the forward just run is 0: its similarity takes no part in the loss, so the tap's backward launches nothing"""
        if self._sf_tap is not None:
            self._sf_tap.cutoff = True

    def set_internal_guidance(self, block_index):
        """Internal Guidance (helpers/training/internal_guidance.py; the reference captures `layer_{i}` at sd3/transformer.py:872): the 0-based joint block whose
        image-stream output feeds the auxiliary head LayerNorm -> Linear(D -> 64).  Call it before `add_lora_adapter` (the head's fp32 masters go to the tail of the
        adapter arena); a full fine-tune needs the constructor's `internal_guidance_block_index` (the head lives inside the base parameter arena, laid out once).
        A training forward then also returns the head's [B, 16, H, W] prediction and the backward takes its gradient at that block."""
        i = internal_guidance_index(block_index, len(self.blocks))
        if self._st_cfg is not None:
            raise NotImplementedError("distillation_method=self_transcendence together with LayerSync / Internal Guidance / NextLat / Self-Flow is not built on the st355 "
                                      "path (they claim the same arena tail)")
        if self._sf_block is not None:
            raise NotImplementedError("crepa_enabled (self_flow) together with Internal Guidance is not built on the st355 path (both claim the tail of the arena that trains)")
        if self._nl_block is not None:
            raise NotImplementedError("Internal Guidance together with NextLat is not built on the st355 path (both heads claim the tail of the arena that trains)")
        if self._ig is not None or self._ig_arena is not None:
            self._ig_block = i                        # the head exists: only the tap moves
            if self._ig is not None:
                self._ig.block = i
            return
        if self.lora_groups or self.full:
            raise RuntimeError("set_internal_guidance: the trainable arena is already laid out without the head — call it before add_lora_adapter(), or construct the "
                               "model with internal_guidance_block_index")
        self._ig_block = i

    def set_nextlat(self, configured_index=None, state_loss: str = "smooth_l1"):
        """NextLat (helpers/training/nextlat.py; the reference captures `layer_{i}` at sd3/transformer.py:872): the joint block whose image-stream output feeds the
        predictor LayerNorm -> Linear(D -> 2D) -> GELU -> Linear(2D -> D), by the reference's rule (`int(configured or -1)`, negative = the last block: None, 0 and -1
        all name the last block).  Call it before `add_lora_adapter` (the predictor's fp32 masters go to the tail of the adapter arena); a full fine-tune needs the
        constructor's `nextlat_block_index` (the predictor lives inside the base parameter arena, laid out once).  A training forward then also returns the state
        loss (mean smooth-L1 / MSE between the prediction from token t and token t + 1) and the backward takes its gradient at that block."""
        if state_loss not in ops.NEXTLAT_MODES:
            raise ValueError("nextlat_state_loss must be 'smooth_l1' or 'mse'.")
        i = nextlat_index(configured_index, len(self.blocks))
        if self._st_cfg is not None:
            raise NotImplementedError("distillation_method=self_transcendence together with LayerSync / Internal Guidance / NextLat / Self-Flow is not built on the st355 "
                                      "path (they claim the same arena tail)")
        if self._sf_block is not None:
            raise NotImplementedError("crepa_enabled (self_flow) together with NextLat is not built on the st355 path (both claim the tail of the arena that trains)")
        if self._ig_block is not None:
            raise NotImplementedError("Internal Guidance together with NextLat is not built on the st355 path (both heads claim the tail of the arena that trains)")
        self._nl_mode = state_loss
        if self._nl is not None or self._nl_arena is not None:
            self._nl_block = i                        # the predictor exists: only the tap moves
            if self._nl is not None:
                self._nl.block = i
            return
        if self.lora_groups or self.full:
            raise RuntimeError("set_nextlat: the trainable arena is already laid out without the predictor — call it before add_lora_adapter(), or construct the "
                               "model with nextlat_block_index")
        self._nl_block = i

    def _nl_head(self) -> NextLatHead:
        if self._nl is None:
            raise RuntimeError("NextLat: no predictor is laid out for training (add_lora_adapter() after set_nextlat(), or enable_full_finetune() on a model "
                               "constructed with nextlat_block_index)")
        return self._nl

    def _ig_head(self) -> InternalGuidanceHead:
        if self._ig is None:
            if self._ig_arena is None:
                raise RuntimeError("Internal Guidance: no head is laid out (add_lora_adapter() after set_internal_guidance(), or the constructor's internal_guidance_block_index)")
            self._ig = InternalGuidanceHead(self._ig_block, self.D, self._ig_arena, (None,) * 4, 0, 0, self.device_)          # inference: the arena's bf16 head, no gradients
        return self._ig

    def set_layersync(self, student_idx, teacher_idx=None):
        """LayerSync (helpers/training/layersync.py; the reference captures at sd3/transformer.py:872): 0-based joint-block indices.  A training forward then also
        returns the mean cosine between the two blocks' image-stream outputs (teacher detached) and the backward adds its gradient into the dX chain at the
        student block."""
        if self._st_cfg is not None:
            raise NotImplementedError("distillation_method=self_transcendence together with LayerSync / Internal Guidance / NextLat / Self-Flow is not built on the st355 "
                                      "path (they claim the same arena tail)")
        if self._sf_block is not None:
            raise NotImplementedError("crepa_enabled (self_flow) together with LayerSync is not built on the st355 path (LayerSync refuses tokenwise timesteps)")
        self._layersync = layersync_indices(student_idx, teacher_idx, len(self.blocks))

    def set_router(self, router, routes):
        """sd3/transformer.py:407-409: TREAD router + [{selection_ratio, start_layer_idx, end_layer_idx}] (training/tread.py)"""
        self._tread_router, self._tread_routes = router, routes

    def _recompute_segment(self, ctx, li: int):
        """backward reached block `li` of a checkpointed segment: re-run the segment's forward from its kept input, this time keeping the activations"""
        s0, n = next((a, c) for (a, c, ck) in ctx.segs if ck and a <= li < a + c)
        img, txt = ctx.ck.pop(s0)
        for bi in range(s0, s0 + n):
            img, txt, ctx.blocks[bi] = self._block_fwd(self.blocks[bi], img, txt, ctx.envs[bi], True)

    def _walk_blocks_bwd(self, ctx, grads, d_taps, taps_kw, block_bwd):
        """the backward walk over the block stack, last block first.  `grads` = [d_img, d_txt] above the last block on entry (d_txt None: the last block is
        context_pre_only), below block 0 on return — a list, here and towards the callee, so that no caller's frame keeps a gradient alive that its consumer is
        done with.  Per block: recompute its checkpointed segment when its activations are gone; the taps' backwards (d_taps: the upstream gradient of each of
        ctx.taps' outputs, taps_kw: (accumulate, sync)) add into d_img at their blocks; a TREAD route is entered at its END — the routed blocks see only the kept
        tokens' gradient rows — and left at its START, where the skipped tokens keep the gradient they had at the route's end;
        `block_bwd(li, blk, sv, env, grads) -> (d_img, d_txt)` does the block's own work: it EMPTIES `grads` as it takes the two, and `sv` (popped from ctx.blocks)
        dies with the call."""
        B, D = ctx.B, self.D
        d_full = None
        for li in range(len(self.blocks) - 1, -1, -1):
            if ctx.blocks[li] is None:
                self._recompute_segment(ctx, li)
            for tap, d in zip(ctx.taps, d_taps):
                if li == tap.block:
                    tap.backward(d, grads[0].view(B, ctx.Si, D), *taps_kw)
            if li in ctx.route_end:
                d_full = grads[0]
                grads[0] = ops.gather_rows(d_full.view(B, ctx.Si, D), ctx.route_end[li].keep_i32()).view(-1, D)
            env, sv = ctx.envs[li], ctx.blocks[li]
            ctx.blocks[li] = None
            grads[:] = block_bwd(li, self.blocks[li], sv, env, grads)
            del sv
            # (a LoRA block 0 through its C entry returns no input gradients — the embedders are frozen: then there is nothing to scatter)
            if li in ctx.route_start and grads[0] is not None:
                ops.scatter_rows(grads[0].view(B, env.Si, D), ctx.route_start[li].keep_i32(), d_full.view(B, ctx.Si, D))
                grads[0], d_full = d_full, None

    def _engine_backward(self, ctx, dout, *d_taps):
        """d_taps: the upstream gradients of the taps' outputs, in ctx.taps' order (LayerSync's similarity, the Internal Guidance prediction, the NextLat state
        loss); each tap's backward takes its own right before its block's own backward"""
        if not self._prepared:
            raise RuntimeError("call prepare_for_training() after loading weights (builds the K-major dgrad operands)")
        D = self.D
        dpk = ops.patchify(dout.to(BF16).contiguous(), order=1).view(ctx.B * ctx.Si, -1)
        mo = ctx.mod_i[:, self.mod_off_out:self.mod_off_out + 2 * D]       # the image stream's modulation rows: per sample, or per token under tokenwise timesteps
        dn = ops.gemm(dpk, self.l_out.wT)
        grads = [ops.ln_modulate_bwd(dn, ctx.x_img_final, mo[:, :D], ctx.rpb_i)[0], None]
        del dn, dpk
        self._walk_blocks_bwd(ctx, grads, d_taps, (self.accumulate_lora_grads, self.grad_sync), lambda li, *a: self._block_bwd(ctx, li, *a))
        return None

    # ------------------------------------------------------------------------------------------------
    # full fine-tune (BASELINE.json configs[3]): every weight, bias and modulation row trains
    # ------------------------------------------------------------------------------------------------
    def _all_linears(self):
        ls = [self.l_patch, self.l_t1, self.l_t2, self.l_p1, self.l_p2, self.l_ctx, self.l_out]
        for blk in self.blocks:
            ls += [l for l in (blk.qkv, blk.add_qkv, blk.to_out, blk.to_add_out, blk.qkv2, blk.to_out2, blk.ff1, blk.ff2, blk.ffc1, blk.ffc2) if l is not None]
        return ls

    def enable_full_finetune(self):
        """gradient arena with the weight arena's layout; every base parameter becomes trainable (bf16 params, bf16 grads)"""
        if self.lora_groups:
            raise RuntimeError("full fine-tune and LoRA adapters are exclusive")
        self.full = True
        # TWO gradient arenas (round 6): the backward fills one and hands it to autograd as it is; the next backward fills the other.  Round 5 cloned the arena at
        # the end of every backward so that `.grad` never aliased the buffer the next backward overwrites (4 GB read + written per SD3-Medium step); with two
        # arenas the hand-over is free, and under gradient accumulation autograd adds the new arena into the one `.grad` still holds (_pick_grad_arena)
        self._grad_arenas = [torch.zeros_like(self.arena), torch.zeros_like(self.arena)]
        self._grad_sel = 0
        self.grad_arena = self._grad_arenas[0]
        base = self.arena.data_ptr()
        self._grad_views = ([], [])          # per arena: (owner, attribute, view) of every gradient view the backward writes through

        def gview(owner, attr, t):
            off = (t.data_ptr() - base) // t.element_size()
            for k in (0, 1):
                self._grad_views[k].append((owner, attr, None if t is None else self._grad_arenas[k][off:off + t.numel()].view(t.shape)))
            setattr(owner, attr, self._grad_views[0][-1][2])

        for l in self._all_linears():
            gview(l, "gw", l.w); gview(l, "gb", l.b)
        for blk in self.blocks:          # q/k RMSNorm weights (SD3.5): gradient views like every other parameter
            for nm in ("norm_q", "norm_k", "norm_added_q", "norm_added_k", "norm_q2", "norm_k2"):
                w = getattr(blk, nm, None)
                if w is not None:
                    gview(blk, "g_" + nm, w)
                else:
                    setattr(blk, "g_" + nm, None)
        gview(self, "g_mod_w", self.mod_w); gview(self, "g_mod_b", self.mod_b)
        if self._ig_block is not None:                # Internal Guidance: the head trains inside the base arena like every other parameter
            if self._ig_arena is None:
                raise RuntimeError("Internal Guidance under a full fine-tune: construct the model with internal_guidance_block_index (the head lives inside the base "
                                   "parameter arena, which is laid out once)")
            lo = (self._ig_arena[0].data_ptr() - base) // self.arena.element_size()
            self._ig = InternalGuidanceHead(self._ig_block, self.D, self._ig_arena, (None,) * 4, lo, self.arena.numel(), self.device_)
            for attr, t in zip(("g_gamma", "g_beta", "g_W", "g_b"), self._ig_arena):
                gview(self._ig, attr, t)
        if self._nl_block is not None:                # NextLat: the predictor trains inside the base arena like every other parameter
            if self._nl_arena is None:
                raise RuntimeError("NextLat under a full fine-tune: construct the model with nextlat_block_index (the predictor lives inside the base parameter arena, "
                                   "which is laid out once)")
            lo = (self._nl_arena[0].data_ptr() - base) // self.arena.element_size()
            self._nl = NextLatHead(self._nl_block, self.D, self._nl_arena, (None,) * 6, lo, self.arena.numel(), self.device_)
            for attr, t in zip(("g_gamma", "g_beta", "g_W_up", "g_b_up", "g_W_down", "g_b_down"), self._nl_arena):
                gview(self._nl, attr, t)
        ps = sorted([p for n, p in self.named_parameters() if ".lora_" not in n and ".lokr_" not in n], key=lambda p: p.data_ptr())
        for p in ps:
            p.requires_grad_(True)
        self._full_params = ps
        self._full_offsets = [((p.data_ptr() - base) // p.element_size(), p.numel()) for p in ps]
        self.prepare_for_training()
        for l in (self.l_t2, self.l_p2):
            l.wT = l.w.t().contiguous()
        return ps

    def _pick_grad_arena(self):
        """before a full fine-tune backward: write into the arena `.grad` does NOT alias (after optimizer.zero_grad(set_to_none=True): either; in the middle of a
        gradient accumulation: the one autograd is not accumulating into)"""
        g = self._full_params[0].grad if self._full_params else None
        if g is not None:
            off0 = self._full_offsets[0][0] * 2
            if g.data_ptr() == self._grad_arenas[self._grad_sel].data_ptr() + off0:
                self._select_grad_arena(1 - self._grad_sel)

    def _select_grad_arena(self, k: int):
        if k == self._grad_sel:
            return
        self._grad_sel = k
        self.grad_arena = self._grad_arenas[k]
        for owner, attr, view in self._grad_views[k]:
            setattr(owner, attr, view)
        if self.grad_sync is not None:
            self.grad_sync.flat = self.grad_arena                     # the exchange walks the arena this backward fills (same offsets)

    def _swap_grad_arena(self):
        """training.grad_sync.hand_over_gradients: the arena just filled now belongs to autograd; the next backward takes the other one"""
        self._select_grad_arena(1 - self._grad_sel)

    def _engine_backward_full(self, ctx, dout, *d_taps):
        """d_taps: as in _engine_backward"""
        D, B, Si, mod = self.D, ctx.B, ctx.Si, ctx.mod
        self._refresh_transposed()
        sync = self.grad_sync
        fb = FullGrads(self, B, self.device_, sync, self._blocks_arena_lo, ctx.emb.st)
        # ---- head ----
        dpk = ops.patchify(dout.to(BF16).contiguous(), order=1).view(B * Si, -1)
        mo = mod[:, self.mod_off_out:self.mod_off_out + 2 * D]
        dmo = fb.dmod[:, self.mod_off_out:self.mod_off_out + 2 * D]
        fb.wgrad(self.l_out, dpk, ctx.n_out)
        dn = ops.gemm(dpk, self.l_out.wT)
        fb.mod_grads(dn, ctx.x_img_final, Si, 1, 0, dmo)                        # AdaLayerNormContinuous: (scale, shift)
        grads = [ops.ln_modulate_bwd(dn, ctx.x_img_final, mo[:, :D], Si)[0], None]
        del dn, dpk
        if sync is not None:
            sync.ready(self._head_arena_lo, self._head_arena_hi)             # proj_out gradients are final (an Internal Guidance head behind it: at its block)
        # the fused modulation matrix (a third of SD3-Medium's parameters, 1.35 GB of gradient) gets its gradient rows block by block (FullGrads.mod_rows_grad)
        fb.mod_rows_grad(self.mod_off_out)                   # norm_out's (scale, shift) rows: final since mod_grads above

        def block_bwd(li, blk, sv, env, grads):
            if li + 1 < len(self.blocks):
                nb = self.blocks[li + 1]
                if sync is not None:
                    sync.ready(nb.arena_lo, nb.arena_hi)                      # the block processed last iteration: its slice can go out
                fb.mod_rows_grad(nb.mod_off)                                     # ... and so can its rows of the modulation matrix
            return self._block_bwd_full(ctx, fb, blk, sv, env, grads)

        self._walk_blocks_bwd(ctx, grads, d_taps, (False, sync), block_bwd)
        d_img, d_txt = grads
        # ---- embedders ----
        em = ctx.emb
        fb.wgrad(self.l_patch, d_img, em.patches)                           # PatchEmbed conv == GEMM on the patches; the position table is a buffer
        fb.wgrad(self.l_ctx, d_txt, em.enc2d)
        dtemb = fb.mod_linear_bwd(em.temb)          # (+ block 0's modulation rows: every other block's went out behind the block after it)
        fb.mlp_bwd(self.l_t1, self.l_t2, em.tproj, em.t1, em.st1, dtemb)
        fb.mlp_bwd(self.l_p1, self.l_p2, em.pooled, em.p1, em.sp1, dtemb)
        fb.ready_front(self.blocks[0].arena_hi)     # embedders, modulation bias, block 0
        return None

    # ------------------------------------------------------------------------------------------------
    # public forward (reference signature: sd3/transformer.py:560-575)
    # ------------------------------------------------------------------------------------------------
    def forward(self, hidden_states, encoder_hidden_states=None, pooled_projections=None, timestep=None, block_controlnet_hidden_states=None,
                joint_attention_kwargs=None, return_dict: bool = True, force_keep_mask=None, return_internal_guidance: bool = False,
                crepa_capture_block_index: Optional[int] = None, crepa_teacher_features=None, self_transcendence_target=None, self_transcendence_sigmas=None,
                **unsupported):
        self._force_keep_mask = force_keep_mask            # TREAD: tokens that may never be routed away (sd3/transformer.py:571, 699-703)
        if block_controlnet_hidden_states is not None:
            raise NotImplementedError("SD3 ControlNet residuals are not wired to the st355 path yet")
        for k, v in unsupported.items():
            if v is not None and v is not False:
                raise NotImplementedError(f"SD3Transformer2DModel(st355): argument {k!r} is not supported on the HIP path")
        if timestep.ndim not in (1, 2):
            raise ValueError(f"timestep: expected [B] or tokenwise [B, S_img], got {tuple(timestep.shape)}")
        need_grad = torch.is_grad_enabled() and (len(self._lora_params) > 0 or getattr(self, "full", False))
        if crepa_capture_block_index is not None:          # Self-Flow's teacher forward: always no-grad, returns `crepa_hidden_states` and no sample
            need_grad = False
        if crepa_teacher_features is not None:             # Self-Flow's training forward: the features its tap aligns to
            if self._sf_block is None or not need_grad:
                raise ValueError("crepa_teacher_features: only a training forward of a component with set_self_flow() takes teacher features")
            self._sf_feats = crepa_teacher_features
        if self_transcendence_target is not None or self_transcendence_sigmas is not None:          # Self-Transcendence's training forward: what its tap is trained to
            if self._st_cfg is None or not need_grad:
                raise ValueError("self_transcendence_target: only a training forward of a component with set_self_transcendence() takes a target")
            self._st_in = (self_transcendence_target, self_transcendence_sigmas)
        if need_grad and not self._prepared and not getattr(self, "full", False):
            self.prepare_for_training()      # K-major dgrad operands went stale (new weights / replica start-state broadcast): rebuild lazily
        if need_grad:      # the training nodes return every tap's output (the similarity / the head's prediction / the state loss) behind the prediction, in the taps' order
            node, params = (_SD3FullFn, self._full_params) if getattr(self, "full", False) else (_SD3Fn, self._lora_params)
            out = node.apply(self, hidden_states, encoder_hidden_states, pooled_projections, timestep, *params)
            out, *rest = out if isinstance(out, tuple) else (out,)
            extra = dict(zip(self._node_keys, rest))
        else:
            with torch.no_grad():
                out, ectx = self._engine_forward(hidden_states.to(BF16), encoder_hidden_states.to(BF16), pooled_projections, timestep, save=False,
                                                 want_ig=bool(return_internal_guidance), capture=crepa_capture_block_index)
                extra = {tap.key: tap.output for tap in ectx.taps}      # sampling: the intermediate prediction next to the final one
        if not return_dict:
            return (out,) + tuple(extra.values())
        return SimpleNamespace(sample=out, **extra)


def _node_outputs(model, out, ctx):
    """what a training node returns: the prediction, then every tap's output; `model._node_keys` names them for `forward`"""
    model._node_keys = [tap.key for tap in ctx.taps]
    return (out, *(tap.output for tap in ctx.taps)) if ctx.taps else out


class _SD3Fn(torch.autograd.Function):
    """one autograd node for the whole network (see flux/transformer.py::_FluxFn)"""

    @staticmethod
    def forward(fctx, model, latents, enc, pooled, timestep, *lora_params):
        out, ctx = model._engine_forward(latents.detach().to(BF16), enc.detach().to(BF16), pooled.detach(), timestep.detach(), save=True)
        fctx.model, fctx.ectx = model, ctx
        return _node_outputs(model, out, ctx)

    @staticmethod
    def backward(fctx, dout, *rest):
        return (None,) * 5 + node_backward(fctx, False, dout, *rest)

class _SD3FullFn(torch.autograd.Function):
    """full fine-tune: one autograd node; backward fills the bf16 gradient arena and hands autograd views of a private copy"""

    @staticmethod
    def forward(fctx, model, latents, enc, pooled, timestep, *params):
        out, ctx = model._engine_forward(latents.detach().to(BF16), enc.detach().to(BF16), pooled.detach(), timestep.detach(), save=True, full=True)
        fctx.model, fctx.ectx = model, ctx
        return _node_outputs(model, out, ctx)

    @staticmethod
    def backward(fctx, dout, *rest):
        fctx.model._pick_grad_arena()
        return (None,) * 5 + node_backward(fctx, True, dout, *rest)
