"""LlavaLlamaForCausalLM for MI355X: the reference's model-level interface over TeoEngine.

Mirrors (names, argument order, defaults, error behaviour):
  language_model/llava_llama.py:40-108  LlavaLlamaForCausalLM.forward / prepare_inputs_for_generation / get_model
  llava_arch.py:125-346                 get_image_tower / encode_images / prepare_inputs_labels_for_multimodal
  generation: the greedy / sampled loop GenerationMixin.generate runs for eval/inference.py:64-72
There is no nn.Module underneath: weights live in the engine's device buffers and all arithmetic is HIP kernels.
The index logic of the embedding splice runs on the host on integers (bit-exact); the data movement is one
teo_embed_splice launch driven by the resulting int32 plan.
"""
from types import SimpleNamespace
from typing import List, Optional

import numpy as np
import torch

from . import _lib as L
from .constants import IGNORE_INDEX, IMAGE_TOKEN_INDEX
from .engine import TeoEngine


class CausalLMOutputWithPast(dict):
    """Minimal stand-in for transformers.modeling_outputs.CausalLMOutputWithPast (attribute + key access)."""

    def __init__(self, loss=None, logits=None, past_key_values=None, hidden_states=None, attentions=None):
        super().__init__(loss=loss, logits=logits, past_key_values=past_key_values, hidden_states=hidden_states,
                         attentions=attentions)
        self.__dict__ = self

    def to_tuple(self):
        return tuple(v for v in (self.loss, self.logits, self.past_key_values, self.hidden_states, self.attentions) if v is not None)


class GenerateOutput(dict):
    """What generate(logprobs=True) returns (attribute + key access): `sequences` is exactly what generate() returns without the keyword;
    `logprobs` fp32 [B, n_new] holds log softmax(logits)[token] of every new token (NaN behind a row's end); `top_token_ids` /
    `top_logprobs` [B, n_new, k] the k most likely tokens of each step, or None with top_logprobs=0."""

    def __init__(self, sequences=None, logprobs=None, top_token_ids=None, top_logprobs=None):
        super().__init__(sequences=sequences, logprobs=logprobs, top_token_ids=top_token_ids, top_logprobs=top_logprobs)
        self.__dict__ = self


def check_logprob_args(logprobs, top_logprobs, prompt_lookup_num_tokens=None):
    """the keyword rules of generate() / generate_batch() / generate_stream(); returns top_logprobs as an int"""
    k = int(top_logprobs or 0)
    if not 0 <= k <= L.LOGPROB_MAX_TOP:
        raise ValueError(f"top_logprobs {k} outside 0..{L.LOGPROB_MAX_TOP}")
    if k and not logprobs:
        raise ValueError("top_logprobs needs logprobs=True")
    if logprobs and prompt_lookup_num_tokens:
        raise ValueError("logprobs=True is not combined with prompt_lookup_num_tokens (the speculative verify step records no log-probabilities)")
    return k


RULE_KEYWORDS = ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "suppress_tokens")


def check_rule_kwargs(kwargs, vocab=None, batch=False):
    """The logit rules of a generate() / generate_batch() / generate_stream() call (include/teo_hip_rules.h): check_rule_args' tuple, or
    None when the four keywords are unset or neutral.  Refuses, before the engine is touched, what has no ruled form."""
    from .decode_host import check_rule_args, rule_args_ban
    rules = check_rule_args(*(kwargs.get(k) for k in RULE_KEYWORDS), vocab=vocab)
    if rules is None:
        return None
    named = ", ".join(k for k in RULE_KEYWORDS if kwargs.get(k) is not None)
    if kwargs.get("prompt_lookup_num_tokens"):
        raise ValueError(f"{named} is not combined with prompt_lookup_num_tokens: the speculative verify step has no form with logit rules")
    if batch:
        raise ValueError(f"{named} applies to one conversation in generate() and not to generate_batch(): generate_stream() applies the "
                         f"rules to any number of requests")
    if rule_args_ban(rules) and (kwargs.get("guide") is not None or kwargs.get("guides") is not None):
        raise ValueError("no_repeat_ngram_size, min_new_tokens and suppress_tokens are not combined with a guide: together they can leave "
                         "a state without an allowed token, which the guide's fallback does not see (repetition_penalty removes no token "
                         "and is allowed)")
    return rules


def _pack_logprobs(entries, k):
    """[(logprobs [n_b], top ids [n_b, k] or None, top logprobs or None)] -> padded [B, n], [B, n, k], [B, n, k] (NaN / -1 behind a row's end)"""
    n = max(int(e[0].numel()) for e in entries)
    lp = torch.full((len(entries), n), float("nan"), dtype=torch.float32)
    ids = torch.full((len(entries), n, k), -1, dtype=torch.int64) if k else None
    tlp = torch.full((len(entries), n, k), float("nan"), dtype=torch.float32) if k else None
    for b, e in enumerate(entries):
        m = int(e[0].numel())
        lp[b, :m] = e[0]
        if k:
            ids[b, :m], tlp[b, :m] = e[1], e[2]
    return lp, ids, tlp


class TeoKVCache:
    """Handle to the engine's device KV cache (one sequence).  `[-1][-1].shape[-2]` reports the cached length so that
    code written against the legacy tuple cache (llava_arch.py:156) keeps working."""

    def __init__(self, engine):
        self.engine = engine

    def get_seq_length(self):
        return self.engine.cache_len

    def __len__(self):
        return self.engine.cfg.num_hidden_layers

    def __getitem__(self, i):
        c = self.engine.cfg
        shape = SimpleNamespace(shape=(1, c.num_key_value_heads, self.engine.cache_len, c.head_dim))
        return (shape, shape)


class TeoBatchKVCache:
    """Handle to the per-conversation device KV caches of a batched forward (the BatchDecoder's slots): what
    forward(input_ids [B, S], use_cache=True) returns at B > 1 and what forward(input_ids [B, 1], past_key_values=...) continues.
    `[-1][-1].shape[-2]` reports the longest cached sequence (the legacy tuple cache of a padded batch has that length,
    llava_arch.py:156)."""

    def __init__(self, engine, decoder):
        self.engine, self.decoder = engine, decoder

    def get_seq_length(self):
        return max(self.decoder.cache_len)

    def __len__(self):
        return self.engine.cfg.num_hidden_layers

    def __getitem__(self, i):
        c = self.engine.cfg
        shape = SimpleNamespace(shape=(self.decoder.B, c.num_key_value_heads, max(self.decoder.cache_len), c.head_dim))
        return (shape, shape)


class TeoImageTower:
    """The tower object `get_image_tower()` returns (LanguageBindImageTower surface, languagebind/__init__.py:94-173)."""

    def __init__(self, engine, processor=None):
        self._engine = engine
        self.is_loaded = True
        self.select_layer = engine.cfg.mm_vision_select_layer
        self.select_feature = engine.cfg.mm_vision_select_feature
        self.image_processor = processor
        self.config = engine.vcfg

    def load_model(self):
        self.is_loaded = True

    def __call__(self, images):
        return self.forward(images)

    def shard_frames(self, comm=None, group=None):
        """Config C4: from now on a batched forward() encodes only this rank's contiguous block of frames and all-gathers
        the visual tokens (teochat_amd/parallel.py).  comm: TeoComm (RCCL behind the C ABI); else torch.distributed `group`."""
        self._shard = (comm, group)

    @torch.no_grad()
    def forward(self, images):
        if type(images) is list:
            return [self._engine.vit_features(im.unsqueeze(0)).to(im.dtype) for im in images]
        shard = getattr(self, "_shard", None)
        if shard is not None:
            from .parallel import sharded_frame_features
            return sharded_frame_features(self._engine.vit_features, images, group=shard[1], comm=shard[0]).to(images.dtype)
        return self._engine.vit_features(images).to(images.dtype)

    @property
    def dtype(self):
        return self._engine.dtype

    @property
    def device(self):
        return self._engine.device

    @property
    def hidden_size(self):
        return self.config.hidden_size

    @property
    def num_patches(self):
        return self.config.num_patches

    @property
    def dummy_feature(self):
        return torch.zeros(1, self.hidden_size, device=self.device, dtype=self.dtype)


class _Projector:
    def __init__(self, engine):
        self._engine = engine

    def __call__(self, x):
        return self._engine.project(x)


class _Embedding:
    def __init__(self, engine):
        self._engine = engine

    @property
    def weight(self):
        return self._engine.embed

    def __call__(self, ids):
        flat = ids.reshape(-1)
        if flat.numel() and (int(flat.min()) < 0 or int(flat.max()) >= self._engine.cfg.vocab_size):
            raise IndexError("index out of range in self")        # what nn.Embedding raises (e.g. a stray -200 sentinel)
        return self._engine.splice(flat.to(torch.int32), None).view(*ids.shape, -1)


class LlavaLlamaModel:
    """`model.model`: holds image_tower / video_tower / mm_projector / embed_tokens like LlavaMetaModel (llava_arch.py:27-49)."""

    def __init__(self, engine, processor=None):
        self.image_tower = TeoImageTower(engine, processor)
        self.video_tower = None
        self.mm_projector = _Projector(engine)
        self.embed_tokens = _Embedding(engine)

    def get_image_tower(self):
        t = getattr(self, "image_tower", None)
        return t[0] if type(t) is list else t

    def get_video_tower(self):
        t = getattr(self, "video_tower", None)
        return t[0] if type(t) is list else t


def build_splice_plan(input_ids, attention_mask, labels, n_feature_rows: List[int], max_length, padding_side):
    """Integer half of prepare_inputs_labels_for_multimodal (llava_arch.py:248-329), on host numpy arrays.

    input_ids [B,n] int64, attention_mask [B,n] bool, labels [B,n] int64, n_feature_rows[i] = rows of image feature i.
    Returns plan [B,Lmax] int32 (>=0 vocab id, <0 -(global visual row)-1, INT32_MIN pad), labels [B,Lmax],
    mask [B,Lmax] bool, position_ids [B,Lmax], lengths.
    Raises IndexError when a sample needs more image features than were supplied (reference: llava_arch.py:284).
    """
    starts = np.concatenate(([0], np.cumsum(n_feature_rows))).astype(np.int64)
    plans, labs = [], []
    nxt = 0                                   # next unused image feature, consumed globally across the batch
    for b in range(input_ids.shape[0]):
        keep = attention_mask[b]
        ids = input_ids[b][keep]
        lab = labels[b][keep]
        if not (ids == IMAGE_TOKEN_INDEX).any():
            if nxt >= len(n_feature_rows):
                raise IndexError("list index out of range")     # the reference indexes image_features[cur_image_idx]
            nxt += 1                          # a text-only sample still consumes one (empty slice of a) feature
            plans.append(ids.astype(np.int64))
            labs.append(lab)
            continue
        p_parts, l_parts = [], []
        cuts = np.flatnonzero(ids == IMAGE_TOKEN_INDEX)
        lo = 0
        for cpos in cuts:
            p_parts.append(ids[lo:cpos].astype(np.int64))
            l_parts.append(lab[lo:cpos])
            if nxt >= len(n_feature_rows):
                raise IndexError("list index out of range")
            rows = np.arange(starts[nxt], starts[nxt + 1], dtype=np.int64)
            p_parts.append(-(rows + 1))
            l_parts.append(np.full(rows.shape[0], IGNORE_INDEX, dtype=lab.dtype))
            nxt += 1
            lo = cpos + 1
        p_parts.append(ids[lo:].astype(np.int64))
        l_parts.append(lab[lo:])
        plans.append(np.concatenate(p_parts))
        labs.append(np.concatenate(l_parts))
    if max_length is not None:
        plans = [p[:max_length] for p in plans]
        labs = [l[:max_length] for l in labs]
    lens = [p.shape[0] for p in plans]
    Lmax = max(lens)
    B = len(plans)
    plan = np.full((B, Lmax), L.INT32_MIN, dtype=np.int64)
    lab_out = np.full((B, Lmax), IGNORE_INDEX, dtype=np.int64)
    mask = np.zeros((B, Lmax), dtype=bool)
    pos = np.zeros((B, Lmax), dtype=np.int64)
    for b, (p, l) in enumerate(zip(plans, labs)):
        n = p.shape[0]
        if n == 0:
            continue
        sl = slice(Lmax - n, Lmax) if padding_side == "left" else slice(0, n)
        plan[b, sl] = p
        lab_out[b, sl] = l
        mask[b, sl] = True
        pos[b, sl] = np.arange(n)
    return plan.astype(np.int32), lab_out, mask, pos, lens


class LlavaLlamaForCausalLM:
    def __init__(self, config, engine: TeoEngine, processor=None):
        self.config = config
        self.engine = engine
        self.model = LlavaLlamaModel(engine, processor)
        self.vocab_size = config.vocab_size
        self.pretraining_tp = getattr(config, "pretraining_tp", 1)
        # HF GenerationConfig defaults; builder.load_generation_config overlays the checkpoint's generation_config.json
        self.generation_config = SimpleNamespace(eos_token_id=getattr(config, "eos_token_id", None), do_sample=False, top_k=50,
                                                 top_p=1.0, temperature=1.0)
        self.training = False
        # {steps, proposed, accepted, emitted} of the last generate(prompt_lookup_num_tokens=K) call; None after any other generate()
        self.last_generation_stats = None

    # --- nn.Module-ish surface the harness touches
    @property
    def device(self):
        return self.engine.device

    @property
    def dtype(self):
        return self.engine.dtype

    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    def get_model(self):
        return self.model

    def get_image_tower(self):
        return self.get_model().get_image_tower()

    def get_video_tower(self):
        return self.get_model().get_video_tower()

    def __call__(self, *a, **k):
        return self.forward(*a, **k)

    # --- H12
    def encode_images(self, images):
        feats = self.get_model().get_image_tower()(images)
        return self.get_model().mm_projector(feats)

    # --- H13
    def prepare_inputs_labels_for_multimodal(self, input_ids, position_ids, attention_mask, past_key_values, labels, images):
        image_tower, video_tower = self.get_image_tower(), self.get_video_tower()
        if (image_tower is None and video_tower is None) or images is None or input_ids.shape[1] == 1:
            if (past_key_values is not None and (image_tower is not None or video_tower is not None)
                    and images is not None and input_ids.shape[1] == 1):
                target = past_key_values[-1][-1].shape[-2] + 1
                pad = torch.ones((attention_mask.shape[0], target - attention_mask.shape[1]),
                                 dtype=attention_mask.dtype, device=attention_mask.device)
                attention_mask = torch.cat((attention_mask, pad), dim=1)
                position_ids = torch.sum(attention_mask, dim=1).unsqueeze(-1) - 1
            return input_ids, position_ids, attention_mask, past_key_values, None, labels

        if any(im.ndim == 4 for im in images):
            raise ValueError("4-D (video) items need a video tower; load_model removes it (eval/eval.py:31)")
        if any(im.ndim != 3 for im in images):
            raise ValueError("images must be a flat list of [3,H,W] tensors")
        if getattr(self.config, "tune_mm_mlp_adapter", False) and getattr(self.config, "mm_use_im_start_end", False):
            raise NotImplementedError

        feats = self.encode_images(torch.stack(list(images)))           # [n_img, NV, D], one batched tower call
        n_img, NV, D = feats.shape
        dev = input_ids.device
        ids_h = input_ids.detach().cpu().numpy()
        mask_h = (np.ones_like(ids_h, dtype=bool) if attention_mask is None
                  else attention_mask.detach().cpu().numpy().astype(bool))
        lab_h = (np.full_like(ids_h, IGNORE_INDEX) if labels is None else labels.detach().cpu().numpy())
        plan, lab_out, mask, pos, _ = build_splice_plan(
            ids_h, mask_h, lab_h, [NV] * n_img, getattr(self.config, "tokenizer_model_max_length", None),
            getattr(self.config, "tokenizer_padding_side", "right"))
        B, Lmax = plan.shape
        embeds = self.engine.splice(torch.from_numpy(plan.reshape(-1)), feats.reshape(n_img * NV, D)).view(B, Lmax, D)
        new_labels = None if labels is None else torch.from_numpy(lab_out).to(dev)
        if attention_mask is None:
            new_mask = None
        else:
            new_mask = torch.from_numpy(mask).to(device=dev, dtype=attention_mask.dtype)
        new_pos = None if position_ids is None else torch.from_numpy(pos).to(device=dev, dtype=position_ids.dtype)
        return None, new_pos, new_mask, past_key_values, embeds, new_labels

    # --- H14 + H15
    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, inputs_embeds=None,
                labels=None, use_cache=None, output_attentions=None, output_hidden_states=None, images=None,
                return_dict=None):
        """LlavaLlamaForCausalLM.forward (llava_llama.py:56-99), same arguments in the same order.

        Contract where it differs from the reference (also in INTEGRATION.md):
          * PADDED positions (attention_mask == 0) are never computed: their `logits` rows and, with `output_hidden_states`, their rows
            in ALL L + 1 hidden-state tensors are ZERO, at B = 1 and at B > 1 alike.  The reference's LlamaModel returns the (masked)
            activations it computed there; a consumer that pools over the full [B, S, D] tensor without applying the attention mask
            gets different values.  Real positions equal the reference's (tests/golden/hidden_*.npz).
          * `output_attentions` (B = 1): one [1, H, S, past + S] map per layer in the model dtype, written by a plain kernel beside the
            unchanged fused forward (teo_llama_prefill_attentions) -- softmax statistics in fp32, one rounding, exact zeros for masked keys;
            at B > 1 or on a batched decode step it raises NotImplementedError.
          * B > 1: `use_cache=True` (explicit) keeps one device cache per conversation and returns a TeoBatchKVCache; the next call
            takes it with input_ids [B, 1] (one batched decode step, every row at its own true next position).  With use_cache
            left None (the training-shape forward) nothing is kept and `past_key_values` is None.
        """
        if inputs_embeds is None:
            (input_ids, position_ids, attention_mask, past_key_values, inputs_embeds, labels) = \
                self.prepare_inputs_labels_for_multimodal(input_ids, position_ids, attention_mask, past_key_values,
                                                          labels, images)
        if inputs_embeds is None:
            inputs_embeds = self.get_model().embed_tokens(input_ids)
        eng = self.engine
        B, S, _ = inputs_embeds.shape
        if output_attentions and (B > 1 or isinstance(past_key_values, TeoBatchKVCache)):
            # the maps come from a plain kernel beside the single-sequence prefill (teo_llama_prefill_attentions); the batched forms keep
            # the fused kernels only
            raise NotImplementedError("output_attentions is a single-sequence feature (B = 1)")
        if isinstance(past_key_values, TeoBatchKVCache):
            # batched continuation (HF generate over a batch re-enters forward with the cache and ONE new token per row,
            # llava_arch.py:154-163): one batched decode step over the BatchDecoder's slots
            return self._forward_batch_step(input_ids, past_key_values, labels, output_hidden_states, return_dict, B, S)
        if past_key_values is None:
            eng.reset_cache()
        elif not isinstance(past_key_values, TeoKVCache) or past_key_values.engine is not eng:
            raise ValueError("past_key_values must be the cache object returned by this model")
        if B > 1 and past_key_values is not None:
            raise ValueError("a one-sequence TeoKVCache cannot continue a batch: pass the TeoBatchKVCache that the batched forward returned")
        past = eng.cache_len
        # B > 1 with use_cache=True (explicitly: the training-shape forward leaves it None and keeps nothing): the prompts are
        # prefilled INTO the batch decoder's per-conversation cache slots and the returned TeoBatchKVCache continues them
        keep_batch = B > 1 and use_cache is True
        logits = torch.zeros(B, S, self.config.vocab_size, dtype=torch.float32, device=eng.device)
        # output_hidden_states (llava_llama.py:56-69 -> LlamaModel.forward): L + 1 tensors [B, S, D] in the model dtype -- the input
        # embeddings, the residual stream after each layer but the last, the final-normed states; padded positions stay zero
        hs_all = (torch.zeros(self.config.num_hidden_layers + 1, B, S, self.config.hidden_size, dtype=eng.dtype, device=eng.device)
                  if output_hidden_states else None)
        # the rows that exist: right / left padding leaves one contiguous run of real tokens per sample (llava_arch.py:310-329); padded
        # positions keep zero logits -- the reference's values there are never consumed (their labels are IGNORE_INDEX, :320-329)
        spans = []
        for b in range(B):
            if attention_mask is not None:
                m = attention_mask[b].to(torch.bool)
                m_new = m[-S:] if m.shape[0] >= S else m
                idx = torch.nonzero(m_new, as_tuple=False).flatten()
                if idx.numel() and int(idx[-1] - idx[0]) + 1 != idx.numel():
                    raise ValueError("attention_mask with holes inside the sequence is not supported")
                if m.shape[0] > S and not bool(m[:-S].all()):
                    raise ValueError("masked positions inside the cached prefix are not supported")
            else:
                idx = torch.arange(S, device=inputs_embeds.device)
            spans.append((int(idx[0]), int(idx[-1]) + 1) if idx.numel() else None)
        if B > 1:
            # every sample in ONE pass: rows of all samples concatenated for the norms / GEMMs, attention per sample on scratch KV
            # slots (teo_llama_prefill_batch).  Positions: 0 .. S_b - 1 per sample (what the default position_ids give; explicit
            # position_ids other than that are a single-sample feature)
            live = [b for b in range(B) if spans[b] is not None]
            if position_ids is not None:
                for b in live:
                    lo, hi = spans[b]
                    pr = position_ids[b] if position_ids.dim() == 2 else position_ids
                    pr = pr[lo:hi] if pr.shape[-1] == S else pr
                    if not torch.equal(pr.to(torch.long).cpu(), torch.arange(hi - lo)):
                        raise ValueError("batched forward supports the default position_ids (0 .. len - 1 per sample) only")
            if keep_batch and len(live) != B:
                raise ValueError("use_cache=True at B > 1 needs at least one real token in every row")
            if live:
                seqs = [inputs_embeds[b, spans[b][0]:spans[b][1]] for b in live]
                if keep_batch:
                    dec = self.batch_decoder(B, 64)
                    dec.reset()
                    out = dec.prefill_all(seqs, last_only=False, hidden_states=hs_all is not None)
                else:
                    out = eng.prefill_batch(seqs, hidden_states=hs_all is not None)
                out, hs = out if hs_all is not None else (out, None)
                r0 = 0
                for b in live:
                    lo, hi = spans[b]
                    logits[b, lo:hi] = out[r0:r0 + hi - lo]
                    if hs is not None:
                        hs_all[:, b, lo:hi] = hs[:, r0:r0 + hi - lo]
                    r0 += hi - lo
        elif spans[0] is not None:
            lo, hi = spans[0]
            pos = None
            if position_ids is not None:
                pr = position_ids[0] if position_ids.dim() == 2 else position_ids
                pos = pr[lo:hi] if pr.shape[-1] == S else pr
            out = eng.prefill(inputs_embeds[0, lo:hi], positions=pos, last_only=False, hidden_states=hs_all is not None,
                              attentions=bool(output_attentions))
            if output_attentions:
                # [layers, H, hi - lo, past + hi - lo] over the real rows; padded query rows / key columns of the caller's [S, past + S]
                # frame stay zero (the contract of padded positions everywhere in this forward)
                att = out[-1]
                out = out[0] if hs_all is None else out[:2]
                att_all = torch.zeros(att.shape[0], 1, att.shape[1], S, past + S, dtype=att.dtype, device=att.device)
                att_all[:, 0, :, lo:hi, :past] = att[..., :past]
                att_all[:, 0, :, lo:hi, past + lo:past + hi] = att[..., past:]
            if hs_all is not None:
                out, hs = out
                hs_all[:, 0, lo:hi] = hs
            logits[0, lo:hi] = out
        pkv = TeoKVCache(eng) if (use_cache is None or use_cache) and B == 1 else None
        if keep_batch:
            pkv = TeoBatchKVCache(eng, self._batch_decoder)
        attn_t = None
        if output_attentions:
            if B == 1 and spans[0] is not None:
                attn_t = tuple(att_all[i] for i in range(att_all.shape[0]))
            else:
                attn_t = tuple(torch.zeros(1, self.config.num_attention_heads, S, past + S, dtype=eng.dtype, device=eng.device)
                               for _ in range(self.config.num_hidden_layers))
        return self._forward_result(logits, labels, pkv, hs_all, return_dict, attn_t)

    def _forward_result(self, logits, labels, pkv, hs_all, return_dict, attentions=None):
        eng = self.engine
        loss = None
        if labels is not None:
            loss = self._shifted_loss(logits, labels)
        out = CausalLMOutputWithPast(loss=loss, logits=logits, past_key_values=pkv, attentions=attentions,
                                     hidden_states=tuple(hs_all[i] for i in range(hs_all.shape[0])) if hs_all is not None else None)
        if return_dict is False:
            return out.to_tuple()
        return out

    def _shifted_loss(self, logits, labels):
        """N4: training-shape loss (CrossEntropyLoss over the shifted positions) on the device: row (b, s) pairs logits[b, s] with
        labels[b, s + 1]; the last position of every sample is ignored."""
        eng = self.engine
        V = self.config.vocab_size
        lab = labels.to(device=logits.device, dtype=torch.int64)
        if bool(((lab != IGNORE_INDEX) & ((lab < 0) | (lab >= V))).any()):
            raise IndexError("Target out of bounds")                    # what torch's cross_entropy reports
        shifted = torch.cat([lab[:, 1:], torch.full_like(lab[:, :1], IGNORE_INDEX)], dim=1).reshape(-1).contiguous()
        rows = shifted.numel()
        loss_row = torch.empty(rows, dtype=torch.float32, device=logits.device)
        out3 = torch.empty(3, dtype=torch.float32, device=logits.device)
        with eng.phase() as st:
            lg = logits.reshape(rows, V)
            L.check(eng.lib.teo_cross_entropy(lg.data_ptr(), V, shifted.data_ptr(), loss_row.data_ptr(), out3.data_ptr(), rows,
                                              V, IGNORE_INDEX, st), "teo_cross_entropy")
        return out3[0]

    def _forward_batch_step(self, input_ids, cache, labels, output_hidden_states, return_dict, B, S):
        """forward(input_ids [B, 1], past_key_values=TeoBatchKVCache): conversation b's new token at ITS OWN next position
        (cache_len[b]); logits [B, 1, V] and the same cache object.  Positions: the reference derives them from the text-level
        attention_mask (sum(mask) - 1, llava_arch.py:157-162), which equals the true next position only when no row of the batch is
        padded; here every row continues at its true length whatever the mask says (stated in INTEGRATION.md)."""
        eng = self.engine
        if cache.engine is not eng or cache.decoder is not getattr(self, "_batch_decoder", None):
            raise ValueError("past_key_values must be the TeoBatchKVCache returned by this model's last batched forward")
        if S != 1 or input_ids is None:
            raise ValueError("batched continuation takes ONE new token id per conversation (input_ids [B, 1])")
        if B != cache.decoder.B:
            raise ValueError(f"the cache holds {cache.decoder.B} conversations, input_ids has {B} rows")
        if output_hidden_states:
            raise NotImplementedError("output_hidden_states on a batched decode step (the fused step keeps no per-layer snapshots)")
        logits = cache.decoder.forward_step(input_ids[:, 0]).view(B, 1, -1)
        return self._forward_result(logits, labels, cache, None, return_dict)

    def prepare_inputs_for_generation(self, input_ids, past_key_values=None, inputs_embeds=None, **kwargs):
        images = kwargs.pop("images", None)
        if past_key_values is not None:
            input_ids = input_ids[:, -1:]
        inputs = {"input_ids": input_ids, "past_key_values": past_key_values, "use_cache": kwargs.get("use_cache"),
                  "attention_mask": kwargs.get("attention_mask")}
        if inputs_embeds is not None and past_key_values is None:
            inputs = {"inputs_embeds": inputs_embeds, **{k: v for k, v in inputs.items() if k != "input_ids"}}
        if images is not None:
            inputs["images"] = images
        return inputs

    # --- H16
    @torch.no_grad()
    def generate(self, *args, **kwargs):
        # one engine phase around the whole call: tower, projector, splice, prefill and the decode chunks run back to back on the
        # engine stream with a single hand-over to the caller's stream at the end (no stream edges between the pieces)
        check_logprob_args(kwargs.get("logprobs"), kwargs.get("top_logprobs"), kwargs.get("prompt_lookup_num_tokens"))
        ids = args[0] if args else kwargs.get("input_ids")
        check_rule_kwargs(kwargs, batch=ids is not None and ids.dim() == 2 and ids.shape[0] != 1)
        with self.engine.phase():
            try:
                return self._generate(*args, **kwargs)
            finally:
                self.engine.guide_end()           # a guide, the recorder and the rules arm the engine's steps for this call only
                self.engine.logprobs_end()
                self.engine.rules_end()

    def _generate(self, input_ids=None, images=None, do_sample=None, temperature=None, top_k=None, top_p=None,
                  max_new_tokens=20, use_cache=True, stopping_criteria=None, eos_token_id="config", attention_mask=None,
                  generator=None, chunk=16, prompt_lookup_num_tokens=None, max_matching_ngram_size=2, prefix_key=None, guide=None, logprobs=False,
                  top_logprobs=0, repetition_penalty=None, no_repeat_ngram_size=None, min_new_tokens=None, suppress_tokens=None, num_beams=None,
                  num_return_sequences=None, length_penalty=None, early_stopping=None, return_dict_in_generate=False, **kwargs):
        """Greedy or sampled (temperature / top-k, device sampler) decoding of ONE sequence; the loop is device-resident
        and replayed from a hipGraph.

        num_beams=B (2..16; HF's keyword and semantics, one conversation), num_return_sequences=n <= B, length_penalty (1.0),
        early_stopping (False / True / "never"): greedy beam search inside the device loop (include/teo_hip_beam.h, teochat_amd/beam.py).
        The beams are the slots of the batched decode step; each step selects the next beams over B x V accumulated scores and makes
        every beam's KV tail the tail of the beam it descends from, on the device; the host looks at one flag per chunk of replays.
        Returns int64 [n, prompt + longest], best first, shorter rows filled with pad_token_id (else EOS); with
        return_dict_in_generate=True a BeamOutput(sequences, sequences_scores).  `last_generation_stats` = {beam_steps, finished,
        reorder_rows}.  Not combined with do_sample, a batch, prompt_lookup_num_tokens, guide, logprobs, prefix_key, the logit rules, custom
        stopping criteria or several distinct stop sequences.  Unset or 1: nothing changes and nothing is allocated.

        prompt_lookup_num_tokens=K (1..15; HF's keyword, one conversation only): prompt-lookup speculative decoding -- every pass over the
        weights verifies the pending token and up to K drafts copied from behind the most recent earlier occurrence of the last
        max_matching_ngram_size (.. 1) tokens (teochat_amd/speculative.py).  The tokens do not depend on the drafts; the weights stream
        through the batched step's kernels.  `last_generation_stats` holds {steps, proposed, accepted, emitted} afterwards: the DEVICE's
        totals -- when a host-side criterion (several stop candidates, a custom StoppingCriteria) ends the call inside a chunk of replays
        they include the steps and tokens the device ran behind that token.  Any other generate() call sets it to None.  0 or None: off.

        prefix_key=k (a hashable; one conversation, not with prompt_lookup_num_tokens): the multi-turn form of prefix reuse.  The model
        remembers the key, the ids and the rows per id of what the engine cache holds after this call; the next generate(prefix_key=k)
        whose ids extend it -- everything up to the last <image>, within the rows the PREFILL wrote (rows appended by decode steps
        carry other kernels' bits), at least one id left -- prefills only the rest behind those rows and skips the tower (`images` is
        not read).  Equal keys promise equal frames.  Any other generate() call, and anything that resets or prefills the engine
        cache, forgets the record.  `last_generation_stats` = {prefix_rows_reused, prefill_rows} afterwards.

        guide=g (a teochat_amd.guide.TokenGuide over this model's vocabulary; one conversation, not with prompt_lookup_num_tokens):
        guided decoding.  Every token -- the first one, which the host path selects from the prefill logits, and those of the device
        loop -- is selected among the tokens the automaton allows in its current state (the others' logits are -inf before argmax / the
        sampler; engine.d_logits holds the masked row afterwards), inside the step's tail kernel (include/teo_hip_guide.h), so the
        loop stays device-resident.  EOS stays the stop; the guide decides when EOS is allowed, and `max_new_tokens` may still cut the
        answer in the middle of the pattern.  Works with prefix_key (nothing in the prefix path reads the guide).
        `last_generation_stats` gains guide_states and guide_table_bytes.

        logprobs=True (not with prompt_lookup_num_tokens), top_logprobs=k (0..8): returns a GenerateOutput instead of the ids tensor --
        `sequences` is that tensor, `logprobs` [B, n_new] the natural-log probability the model gave each new token, the stop token
        included, `top_token_ids` / `top_logprobs` [B, n_new, k] the k most likely tokens of each step (None with k = 0).  The value is
        log softmax(logits)[token]: temperature, top_k and top_p do not enter.  One more launch behind each decode step records it on the
        device (include/teo_hip_logprob.h); the first token's entry comes from the prefill logits.  Under a guide the row is the masked
        one, so the value is the probability AMONG THE TOKENS THE GUIDE ALLOWED.  With the keyword unset nothing changes.

        repetition_penalty=p, no_repeat_ngram_size=n, min_new_tokens=m, suppress_tokens=[ids] (HF's keywords and semantics; one
        conversation, not with prompt_lookup_num_tokens; None / 1.0 / 0 / [] = off): logit rules over the prompt ids as passed (a -200
        sentinel is an ordinary id that addresses no logit) followed by the tokens emitted so far, applied by one more launch between each
        step's lm_head and its tail (include/teo_hip_rules.h) -- before the guide's mask, argmax or the sampler, and before the recorder,
        so engine.d_logits and `logprobs` hold the processed row.  The first token goes through the same kernel on the prefill row.
        min_new_tokens bans `eos_token_id` only.  The three banning rules are not combined with a guide; repetition_penalty is.  A row
        left without a finite logit selects what the tail selects there (greedy: token 0).  `last_generation_stats` gains the rules in
        force.  With the four keywords unset nothing is allocated and the existing graphs replay.

        Returns int64 [1, n_prompt + n_generated]; the prompt part still contains the -200 sentinels, as with the
        reference (eval/inference.py:75 slices at input_ids.shape[1]).  `eos_token_id=None` disables EOS stopping.
        """
        # unspecified sampling knobs come from the checkpoint's generation_config.json (HF GenerationMixin semantics)
        gc = self.generation_config
        do_sample = bool(getattr(gc, "do_sample", False)) if do_sample is None else do_sample
        temperature = float(getattr(gc, "temperature", 1.0) or 1.0) if temperature is None else temperature
        top_k = getattr(gc, "top_k", 50) if top_k is None else top_k
        top_p = getattr(gc, "top_p", 1.0) if top_p is None else top_p
        self.last_generation_stats = None
        K = int(prompt_lookup_num_tokens or 0)
        top_n = check_logprob_args(logprobs, top_logprobs, K)
        rules = check_rule_kwargs(dict(repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                                       min_new_tokens=min_new_tokens, suppress_tokens=suppress_tokens, prompt_lookup_num_tokens=K, guide=guide),
                                  vocab=self.engine.cfg.vocab_size, batch=input_ids.shape[0] != 1)
        from .beam import check_beam_args
        beam = check_beam_args(getattr(gc, "num_beams", 1) if num_beams is None else num_beams,
                               getattr(gc, "num_return_sequences", 1) if num_return_sequences is None else num_return_sequences,
                               getattr(gc, "length_penalty", 1.0) if length_penalty is None else length_penalty,
                               getattr(gc, "early_stopping", False) if early_stopping is None else early_stopping, do_sample=do_sample)
        if beam is not None:
            self._prefix_record = None
            for given, name in ((input_ids.shape[0] != 1, "a batch of conversations (num_beams applies to one conversation)"),
                                (K, "prompt_lookup_num_tokens"), (guide is not None, "guide"), (logprobs, "logprobs"),
                                (prefix_key is not None, "prefix_key"), (rules is not None, "the logit rules (repetition_penalty, "
                                 "no_repeat_ngram_size, min_new_tokens, suppress_tokens)")):
                if given:
                    raise ValueError(f"num_beams is not combined with {name}")
            return self._generate_beam(input_ids, images, attention_mask, max_new_tokens, eos_token_id, stopping_criteria, chunk, beam,
                                       return_dict_in_generate)
        if K and prefix_key is not None:
            raise ValueError("prefix_key is not combined with prompt_lookup_num_tokens")
        record, self._prefix_record = getattr(self, "_prefix_record", None), None          # any generate() call forgets it
        if K and not 1 <= K <= 15:
            raise ValueError(f"prompt_lookup_num_tokens {K} outside 1..15")
        if K and input_ids.shape[0] != 1:
            raise ValueError("prompt_lookup_num_tokens applies to one conversation (batch 1)")
        if guide is not None and K:
            raise ValueError("guide is not combined with prompt_lookup_num_tokens")
        if guide is not None and input_ids.shape[0] != 1:
            raise ValueError("guide applies to one conversation (batch 1); generate_stream(guides=...) takes one guide per request")
        if guide is not None and guide.vocab != self.engine.cfg.vocab_size:
            raise ValueError(f"the guide's table is {guide.vocab} tokens wide, the model's vocabulary {self.engine.cfg.vocab_size}")
        if input_ids.shape[0] != 1:
            # batch of conversations: rows are cut by attention_mask, `images` is a list with one entry per conversation
            B = input_ids.shape[0]
            rows = [input_ids[b][attention_mask[b].to(torch.bool)] if attention_mask is not None else input_ids[b]
                    for b in range(B)]
            if images is not None and (not isinstance(images, (list, tuple)) or len(images) != B):
                raise ValueError("batched generate(): `images` must be a list with one entry (frame list) per conversation")
            outs = self.generate_batch(rows, images, do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p,
                                       max_new_tokens=max_new_tokens, stopping_criteria=stopping_criteria,
                                       eos_token_id=eos_token_id, generator=generator, chunk=chunk, logprobs=logprobs, top_logprobs=top_n)
            entries = None
            if logprobs:
                outs, entries = [o[0] for o in outs], [o[1:] for o in outs]
            # what GenerationMixin.generate returns: the input rows exactly as given (left or right padding included) followed
            # by the new tokens of each row; rows that stopped early are filled up with pad_token_id
            pad = getattr(self.config, "pad_token_id", None)
            pad = 0 if pad is None else int(pad)
            news = [o[rows[b].numel():] for b, o in enumerate(outs)]
            n_new = max(int(t.numel()) for t in news)
            tail = torch.full((B, n_new), pad, dtype=input_ids.dtype, device=input_ids.device)
            for b, t in enumerate(news):
                tail[b, :t.numel()] = t.to(tail.device)
            seqs = torch.cat([input_ids, tail], dim=1)
            return GenerateOutput(seqs, *_pack_logprobs(entries, top_n)) if logprobs else seqs
        eng = self.engine
        if eos_token_id == "config":
            eos_token_id = self._config_eos()
        crits = list(stopping_criteria or [])
        if max_new_tokens <= 0:
            if logprobs:
                z = torch.zeros(1, 0, top_n)
                return GenerateOutput(input_ids, torch.zeros(1, 0), z.to(torch.int64) if top_n else None, z if top_n else None)
            return input_ids
        # ---- prefill
        ids_t, reuse = tuple(input_ids[0].tolist()), (0, 0)
        plain_mask = attention_mask is None or bool(attention_mask.to(torch.bool).all())
        if prefix_key is not None and record is not None and plain_mask and record[0] == prefix_key and record[4] == getattr(eng, "cache_epoch", 0):
            from .stream import reusable_prefix
            reuse = reusable_prefix(ids_t, record[:4], 1)
            if reuse[0] != len(record[1]):          # the next turn EXTENDS the remembered prompt; anything else takes the full path
                reuse = (0, 0)
        if reuse[1]:
            embeds = self.get_model().embed_tokens(input_ids[:, reuse[0]:])       # text ids only: no tower, `images` is not read
            row_map = tuple(record[2][:reuse[0]]) + (1,) * (len(ids_t) - reuse[0])
        else:
            (_, pos, mask, _, embeds, _) = self.prepare_inputs_labels_for_multimodal(input_ids, None, attention_mask, None,
                                                                                   None, images)
            if embeds is None:
                embeds = self.get_model().embed_tokens(input_ids)
            n_img = sum(1 for t in ids_t if t < 0)
            nv = (int(embeds.shape[1]) - (len(ids_t) - n_img)) // n_img if n_img else 0
            row_map = tuple(nv if t < 0 else 1 for t in ids_t)
            if not plain_mask or sum(row_map) != int(embeds.shape[1]):
                row_map = None                      # rows cut by a mask or by tokenizer_model_max_length: nothing to remember
        spec = None
        if K:
            # one verify step writes K + 1 cache rows from the pending token's position on, whatever it accepts
            if embeds.shape[1] + max_new_tokens - 1 + K + 1 > eng.max_seq:
                raise ValueError(f"prompt ({embeds.shape[1]}) + max_new_tokens ({max_new_tokens}) - 1 + prompt_lookup_num_tokens + 1 "
                                 f"({K + 1}) exceeds max_seq {eng.max_seq}")
            spec = self.spec_decoder(K + 1, max_new=max_new_tokens, ngram_max=int(max_matching_ngram_size)) if max_new_tokens > 1 else None
        if spec is not None:
            spec.reset()
            logits = spec.prefill(embeds[0], last_only=True)
        else:
            if reuse[1] + embeds.shape[1] + max_new_tokens > eng.max_seq:
                raise ValueError(f"prompt ({reuse[1] + embeds.shape[1]}) + max_new_tokens ({max_new_tokens}) exceeds max_seq {eng.max_seq}")
            if reuse[1]:
                eng.cache_len = reuse[1]            # the rows the last generate(prefix_key=) prefilled stay; the rest follows behind them
            else:
                eng.reset_cache()
            logits = eng.prefill(embeds[0], last_only=True)
            if prefix_key is not None:
                self.last_generation_stats = dict(prefix_rows_reused=reuse[1], prefill_rows=int(embeds.shape[1]))
                if row_map is not None:             # (key, ids, rows per id, rows written by prefill, the cache's epoch)
                    self._prefix_record = (prefix_key, ids_t, row_map, eng.cache_len, eng.cache_epoch)
        if rules is not None:
            # the rules' state starts from the prompt ids as passed; the first token comes from the prefill row through the same kernel
            eng.rules_begin(1, rules, eos_ids=[eos_token_id] if eos_token_id is not None else [])
            eng.rules_seed(0, input_ids[0])
            logits = logits.contiguous()
            eng.rules_first(logits[0])
            self.last_generation_stats = dict(self.last_generation_stats or {}, **eng.rules_in_force(), suppress_tokens=len(rules[3]))
        if guide is not None:
            eng.guide_begin(guide)
            logits = logits.contiguous()
            eng.guide_mask(logits[:1])             # the first token comes from the prefill logits: the same mask, the same state
            self.last_generation_stats = dict(self.last_generation_stats or {}, guide_states=int(guide.n_states),
                                              guide_table_bytes=int(guide.table_bytes))
        if do_sample:
            tp = 1.0 if top_p is None else float(top_p)
            k = int(top_k or 0)                    # 0 = top-k filter off (HF: top_k=0 / None disables TopKLogitsWarper)
            seed = generator.initial_seed() if generator is not None else int(torch.randint(0, 2 ** 62, (1,)).item())
            first = eng.sample(logits[0], temperature, k, seed, 0, top_p=tp)
        else:
            k, seed, tp = 0, 0, 1.0
            first = self._argmax(logits[0])
        first_lp = None
        if logprobs:
            # the first token's entry: the prefill row it was selected from (masked, under a guide), through the recorder's own body
            from .decode_host import logprob_rows
            first_lp = [t.cpu() for t in logprob_rows(eng, logits[:1].contiguous(), [first], top_n)]
            eng.logprobs_begin(top_n)
        if guide is not None:
            eng.guide_advance([first])
        new_tokens = [first]

        def finish(tokens):
            seqs = self._finish(input_ids, tokens)
            if not logprobs:
                return seqs
            lp, ids, tlp = first_lp
            if len(tokens) > 1:
                r = eng.recorded(0, len(tokens) - 1)
                lp = torch.cat([lp, r[0]])
                if top_n:
                    ids, tlp = torch.cat([ids, r[1]]), torch.cat([tlp, r[2]])
            return GenerateOutput(seqs, lp.view(1, -1), ids.unsqueeze(0) if top_n else None, tlp.unsqueeze(0) if top_n else None)

        def done(tokens):
            if eos_token_id is not None and tokens[-1] == eos_token_id:
                return True
            if crits:
                row = torch.cat([input_ids[0].cpu(), torch.tensor(tokens, dtype=torch.long)]).unsqueeze(0)
                return any(bool(c(row, None)) for c in crits)
            return False

        if done(new_tokens) or max_new_tokens == 1:
            return finish(new_tokens)
        # ---- decode: the whole loop (incl. the sampler) runs on the device, replayed from a hipGraph in chunks;
        # the host only looks at the tokens once per chunk to apply EOS / stopping criteria at the exact token.
        cands = [ids for c in crits for ids in getattr(c, "keyword_id_lists", []) if ids]
        if eos_token_id is not None:
            cands.append([int(eos_token_id)])
        # the reference's default call stops on the keyword "</s>" AND on EOS (eval/inference.py:57-72), which are the same id
        # sequence [2]: duplicates are folded so that this default arms the device-side stop
        uniq = []
        for ids in cands:
            ids = [int(t) for t in ids]
            if ids not in uniq:
                uniq.append(ids)
        stop_ids = uniq[0] if len(uniq) == 1 else None
        if spec is not None:
            # verify steps: the same device-resident loop, up to K + 1 tokens per replay; the host looks once per chunk of replays
            spec.begin(first, input_ids[0].tolist() + [first], stop_ids, do_sample=do_sample, temperature=temperature, top_k=k, seed=seed,
                       draws_done=1, top_p=tp, max_new=max_new_tokens - 1)
            stop_here = False
            while not stop_here and len(new_tokens) < max_new_tokens:
                spec.steps(chunk)
                got = spec.generated().tolist()
                for t in got[len(new_tokens) - 1:]:
                    new_tokens.append(int(t))
                    if done(new_tokens):
                        stop_here = True
                        break
                stop_here = stop_here or spec.stopped()
            self.last_generation_stats = spec.stats()
            return self._finish(input_ids, new_tokens)
        eng.decode_begin(first, stop_ids, do_sample=do_sample, temperature=temperature, top_k=k, seed=seed, draws_done=1, top_p=tp)
        remaining = max_new_tokens - 1
        while remaining > 0:
            n = min(chunk, remaining)
            eng.decode_steps(n, use_graph=True)
            got = eng.generated().tolist()
            fresh = got[len(new_tokens) - 1:]
            stop_here = False
            for t in fresh:
                new_tokens.append(int(t))
                remaining -= 1
                if done(new_tokens):
                    stop_here = True
                    break
            if stop_here:
                break
        return finish(new_tokens)

    def beam_decoder(self, num_beams, max_new=1024):
        """the beam state over the model's B-slot stream decoder (its caches and weight copies: no second set)"""
        from .beam import BeamDecoder
        dec = self.stream_decoder(num_beams, max_new)
        cur = getattr(self, "_beam_decoder", None)
        if cur is None or cur.dec is not dec or cur.cap < max_new:
            self._beam_decoder = None
            cur = BeamDecoder(dec, max(int(max_new), dec.max_new))
            self._beam_decoder = cur
        return cur

    def _generate_beam(self, input_ids, images, attention_mask, max_new_tokens, eos_token_id, stopping_criteria, chunk, beam,
                       return_dict):
        """generate(num_beams=B): see _generate"""
        from .beam import BeamOutput
        B, n_ret, lp, es = beam
        eng = self.engine
        if eos_token_id == "config":
            eos_token_id = self._config_eos()
        # the stop: EOS and the reference's default keyword "</s>" are the same single id; anything else has no form in the device loop
        cands = []
        for c in list(stopping_criteria or []):
            lists = [ids for ids in getattr(c, "keyword_id_lists", []) if ids]
            if not lists:
                raise ValueError("num_beams is not combined with custom stopping_criteria: the search stops on one EOS id")
            cands += lists
        if eos_token_id is not None:
            cands.append([int(eos_token_id)])
        uniq = []
        for ids in cands:
            ids = [int(t) for t in ids]
            if ids not in uniq:
                uniq.append(ids)
        if len(uniq) > 1 or (uniq and len(uniq[0]) != 1):
            raise ValueError(f"num_beams is not combined with several distinct stop sequences or a stop of several ids: {uniq}")
        eos = uniq[0][0] if uniq else None
        if max_new_tokens <= 0:
            return BeamOutput(input_ids, torch.zeros(1)) if return_dict else input_ids
        if input_ids.shape[1] + max_new_tokens > eng.max_seq:
            raise ValueError(f"prompt ({input_ids.shape[1]} ids) + max_new_tokens ({max_new_tokens}) exceeds max_seq {eng.max_seq}")
        (_, _, _, _, embeds, _) = self.prepare_inputs_labels_for_multimodal(input_ids, None, attention_mask, None, None, images)
        if embeds is None:
            embeds = self.get_model().embed_tokens(input_ids)
        if embeds.shape[1] + max_new_tokens > eng.max_seq:
            raise ValueError(f"prompt ({embeds.shape[1]}) + max_new_tokens ({max_new_tokens}) exceeds max_seq {eng.max_seq}")
        bm = self.beam_decoder(B, max_new_tokens)
        try:
            bm.begin(embeds[0], eos=eos, max_new=max_new_tokens, length_penalty=lp, early_stopping=es)
            bm.run(chunk)
            hyps, stats = bm.finish(n_ret)
        finally:
            bm.end()
        self.last_generation_stats = stats
        pad = getattr(self.config, "pad_token_id", None)
        fill = (pad or eos) if eos is not None else -1            # HF's fill rule
        longest = max(len(h) for _, h in hyps)
        tail = torch.full((len(hyps), longest), int(fill), dtype=input_ids.dtype)
        for i, (_, h) in enumerate(hyps):
            tail[i, :len(h)] = torch.tensor(h, dtype=input_ids.dtype)
        seqs = torch.cat([input_ids.expand(len(hyps), -1), tail.to(input_ids.device)], dim=1)
        if not return_dict:
            return seqs
        return BeamOutput(seqs, torch.stack([s for s, _ in hyps]).to(torch.float32))

    # --- closed-set answers: log p(option | frames, question) of every option, the options packed into one pass over the weights
    @torch.no_grad()
    def score_options(self, input_ids, images, options, attention_mask=None, max_rows=1024):
        """fp32 [N] on the model device: for each option (a list of token ids) the sum over its tokens of the natural-log probability
        given the prompt and the option's earlier tokens.  One conversation.  Tower, projector, splice and the prompt's prefill run as in
        generate(); then the options' rows are scored as packed branches of the cached prompt (score.plan_branches,
        teo_llama_prefill_branches): one pass over the weights per `max_rows` rows instead of one per option.  The token log-probs come
        from teo_token_logprobs in fp32; the per-option sum is taken in fp64 on the host.  Forgets the prefix_key record like any
        generate() call; `last_generation_stats` = {prompt_rows, branch_rows, passes} afterwards."""
        from .score import PROMPT_ROW, plan_branches
        if input_ids.dim() != 2 or input_ids.shape[0] != 1:
            raise ValueError("score_options applies to one conversation (input_ids [1, n])")
        option_ids = [[int(t) for t in (o.tolist() if hasattr(o, "tolist") else o)] for o in options]
        V = self.engine.cfg.vocab_size
        for c, ids in enumerate(option_ids):
            if not ids or min(ids) < 0 or max(ids) >= V:
                raise ValueError(f"score_options: option {c} is empty or holds ids outside 0..{V - 1}")
        self.last_generation_stats = None
        self._prefix_record = None
        eng = self.engine
        with eng.phase():
            (_, pos, mask, _, embeds, _) = self.prepare_inputs_labels_for_multimodal(input_ids, None, attention_mask, None, None, images)
            if embeds is None:
                embeds = self.get_model().embed_tokens(input_ids)
            P = int(embeds.shape[1])
            if option_ids and P + 1 > eng.max_seq:
                raise ValueError(f"prompt ({P}) leaves no room behind it in max_seq {eng.max_seq}")
            passes = plan_branches(option_ids, P, eng.max_seq, max_rows) if option_ids else []
            eng.reset_cache()
            prompt_logits = eng.prefill(embeds[0], last_only=True)
            totals = [0.0] * len(option_ids)
            branch_rows = 0
            for p in passes:
                S = len(p["rows"])
                branch_rows += S
                firsts = [t for t in p["triples"] if t[0] == PROMPT_ROW]
                rest = [t for t in p["triples"] if t[0] != PROMPT_ROW]
                lp = eng.token_logprobs(prompt_logits, [0] * len(firsts), [t[1] for t in firsts]).tolist()
                for t, v in zip(firsts, lp):
                    totals[t[2]] += v
                if S:
                    rows = self.get_model().embed_tokens(torch.tensor(p["rows"], dtype=torch.long, device=input_ids.device).view(1, -1))[0]
                    logits = eng.prefill_branches(rows, p["positions"], p["branch_start"])
                    lp = eng.token_logprobs(logits, [t[0] for t in rest], [t[1] for t in rest]).tolist()
                    for t, v in zip(rest, lp):
                        totals[t[2]] += v
        self.last_generation_stats = dict(prompt_rows=P, branch_rows=branch_rows, passes=len(passes))
        return torch.tensor(totals, dtype=torch.float64).to(torch.float32).to(eng.device)

    # --- speculative verify steps (prompt lookup): R rows of one conversation per pass over the weights
    def spec_decoder(self, rows, max_new=1024, ngram_max=2):
        from .speculative import SpecDecoder
        w4 = bool(self.engine.batch_mxfp4)
        cur = getattr(self, "_spec_decoder", None)
        if cur is None or cur.R != rows or cur.max_new < max_new or cur.ngram_max != ngram_max or cur.w4_requested != w4:
            self._spec_decoder = None           # free the old cache first
            bd = getattr(self, "_batch_decoder", None)
            if bd is not None and bd.w4_requested != w4:
                bd = None                       # (its copies are in the other weight format)
            cur = SpecDecoder(self.engine, rows, max_new=max(max_new, 64), ngram_max=ngram_max, batch_decoder=bd)
            self._spec_decoder = cur
        return cur

    # --- batched decode (config C5's variant): B conversations, one pass over the weights per generated token
    def batch_decoder(self, batch, max_new=1024):
        from .batch import BatchDecoder
        cur = getattr(self, "_batch_decoder", None)
        if cur is None or cur.B != batch or cur.max_new < max_new or cur.w4_requested != bool(self.engine.batch_mxfp4):
            self._batch_decoder = None          # free the old caches first
            cur = BatchDecoder(self.engine, batch, max_new=max(max_new, 64))
            self._batch_decoder = cur
        return cur

    @torch.no_grad()
    def generate_batch(self, *args, **kwargs):
        check_logprob_args(kwargs.get("logprobs"), kwargs.get("top_logprobs"))
        check_rule_kwargs(kwargs, batch=True)     # (any rule is refused here; neutral values pass and are dropped)
        kwargs = {k: v for k, v in kwargs.items() if k not in RULE_KEYWORDS}
        with self.engine.phase():
            return self._generate_batch(*args, **kwargs)

    def _generate_batch(self, input_ids_list, images_list=None, do_sample=False, temperature=None, top_k=None, top_p=None,
                        max_new_tokens=20, stopping_criteria=None, eos_token_id="config", generator=None, chunk=16, logprobs=False,
                        top_logprobs=0):
        """Decode B conversations together (B <= 16).  input_ids_list: B 1-D id tensors (with -200 sentinels);
        images_list: per conversation what generate() takes as `images`.  stopping_criteria: None, or one list of
        criteria per conversation.  Returns B 1-D tensors prompt + generated, each cut at its own EOS / stop keyword.

        One multimodal preparation and ONE prefill pass over the concatenated rows of all conversations (per-sequence RoPE,
        KV append and causal attention); the decode loop is batched: per step every weight matrix is streamed once for all
        conversations (teo_llama_decode_batch_step).

        logprobs=True, top_logprobs=k: every entry of the returned list is (ids, logprobs [n_new], top ids [n_new, k] or None, top
        logprobs or None) instead of the ids tensor, as generate_stream(logprobs=True) returns them (see generate())."""
        top_n = check_logprob_args(logprobs, top_logprobs)
        B = len(input_ids_list)
        if eos_token_id == "config":
            eos_token_id = self._config_eos()
        if max_new_tokens <= 0:
            if logprobs:
                z = torch.zeros(0, top_n)
                return [(ids.clone(), torch.zeros(0), z.to(torch.int64) if top_n else None, z if top_n else None) for ids in input_ids_list]
            return [ids.clone() for ids in input_ids_list]
        gc = self.generation_config
        temperature = float(getattr(gc, "temperature", 1.0) or 1.0) if temperature is None else temperature
        top_k = getattr(gc, "top_k", 50) if top_k is None else top_k
        top_p = getattr(gc, "top_p", 1.0) if top_p is None else top_p
        tp = 1.0 if (top_p is None or not do_sample) else float(top_p)
        crits = list(stopping_criteria) if stopping_criteria is not None else [[] for _ in range(B)]
        if len(crits) != B:
            raise ValueError("stopping_criteria must hold one list per conversation")
        eng = self.engine
        dec = self.batch_decoder(B, max_new_tokens)
        dec.reset()
        k = int(top_k or 0) if do_sample else 0
        base_seed = 0
        if do_sample:
            base_seed = generator.initial_seed() if generator is not None else int(torch.randint(0, 2 ** 62, (1,)).item())
        seeds = [(base_seed + 0x9E3779B97F4A7C15 * b) & (2 ** 63 - 1) for b in range(B)]
        # one multimodal preparation for the whole batch: every frame of every conversation goes through the tower and
        # the projector in ONE call (flat image list consumed in order, llava_arch.py:284-285), one splice launch
        dev_ids = input_ids_list[0].device
        width = max(int(ids.numel()) for ids in input_ids_list)
        ids_p = torch.zeros(B, width, dtype=torch.long, device=dev_ids)
        mask_p = torch.zeros(B, width, dtype=torch.long, device=dev_ids)
        for b, ids in enumerate(input_ids_list):
            ids_p[b, :ids.numel()] = ids.view(-1)
            mask_p[b, :ids.numel()] = 1
        flat = []
        for b in range(B):
            imgs = images_list[b] if images_list is not None else None
            if imgs is not None:
                flat.extend(list(imgs))
        (_, _, new_mask, _, embeds, _) = self.prepare_inputs_labels_for_multimodal(ids_p, None, mask_p, None, None, flat or None)
        if embeds is None:
            embeds, new_mask = self.get_model().embed_tokens(ids_p), mask_p
        seqs = []
        for b in range(B):
            rows = torch.nonzero(new_mask[b].to(torch.bool), as_tuple=False).flatten()
            lo, hi = int(rows[0]), int(rows[-1]) + 1
            if hi - lo + max_new_tokens > eng.max_seq:
                raise ValueError(f"prompt ({hi - lo}) + max_new_tokens ({max_new_tokens}) exceeds max_seq {eng.max_seq}")
            seqs.append(embeds[b, lo:hi])
        logits = dec.prefill_all(seqs)             # one pass over the concatenated rows of all conversations
        firsts = [eng.sample(logits[b], temperature, k, seeds[b], 0, top_p=tp) if do_sample else self._argmax(logits[b])
                  for b in range(B)]
        new_tokens = [[t] for t in firsts]
        finished = [False] * B
        first_lp = None
        if logprobs:
            from .decode_host import logprob_rows
            first_lp = [t.cpu() for t in logprob_rows(eng, logits[:B].contiguous(), firsts, top_n)]
            dec.logprobs_begin(top_n)

        def done(b):
            toks = new_tokens[b]
            if eos_token_id is not None and toks[-1] == eos_token_id:
                return True
            if crits[b]:
                row = torch.cat([input_ids_list[b].cpu().view(-1), torch.tensor(toks, dtype=torch.long)]).unsqueeze(0)
                return any(bool(c(row, None)) for c in crits[b])
            return False

        for b in range(B):
            finished[b] = done(b) or max_new_tokens == 1
        if not all(finished):
            stop_ids = [int(eos_token_id)] if (eos_token_id is not None and not any(crits)) else None
            dec.begin(firsts, stop_ids, do_sample=do_sample, temperature=temperature, top_k=k, seeds=seeds, draws_done=1, top_p=tp)
            remaining = max_new_tokens - 1
            while remaining > 0 and not all(finished):
                n = min(chunk, remaining)
                dec.steps(n, use_graph=True)
                got = dec.generated()[:, -n:].tolist()
                for b in range(B):
                    if finished[b]:
                        continue
                    for t in got[b]:
                        new_tokens[b].append(int(t))
                        if done(b):
                            finished[b] = True
                            break
                remaining -= n
        outs = [torch.cat([input_ids_list[b].view(-1), torch.tensor(new_tokens[b], dtype=input_ids_list[b].dtype,
                                                                     device=input_ids_list[b].device)]) for b in range(B)]
        if not logprobs:
            return outs
        res = []
        for b in range(B):
            lp, ids, tlp = first_lp[0][b:b + 1], first_lp[1][b:b + 1], first_lp[2][b:b + 1]
            if len(new_tokens[b]) > 1:
                r = dec.recorded(b, len(new_tokens[b]) - 1)
                lp = torch.cat([lp, r[0]])
                if top_n:
                    ids, tlp = torch.cat([ids, r[1]]), torch.cat([tlp, r[2]])
            res.append((outs[b], lp, ids if top_n else None, tlp if top_n else None))
        dec.logprobs_end()
        return res

    # --- continuous batching: the batched step over slots that park when they finish and are refilled from a queue of requests
    def stream_decoder(self, slots, max_new=1024):
        from .stream import StreamDecoder
        bd = self.batch_decoder(slots, max_new)   # its caches and weight copies are shared: no second copy of the weights
        cur = getattr(self, "_stream_decoder", None)
        if cur is None or cur.bd is not bd:
            cur = StreamDecoder(self.engine, slots, max_new=bd.max_new, batch_decoder=bd)
            self._stream_decoder = cur
        return cur

    @torch.no_grad()
    def generate_stream(self, *args, **kwargs):
        check_logprob_args(kwargs.get("logprobs"), kwargs.get("top_logprobs"))
        check_rule_kwargs(kwargs)
        with self.engine.phase():
            return self._generate_stream(*args, **kwargs)

    def _generate_stream(self, input_ids_list, images_list=None, slots=8, max_new_tokens=20, do_sample=False, temperature=None,
                         top_k=None, top_p=None, stopping_criteria=None, eos_token_id="config", generator=None, chunk=16, prefix_keys=None,
                         min_prefix_rows=64, guides=None, share_prefix=False, logprobs=False, top_logprobs=0, repetition_penalty=None,
                         no_repeat_ngram_size=None, min_new_tokens=None, suppress_tokens=None):
        """Answer N requests (any N >= 1) over `slots` <= 16 conversation slots of the batched decode step: a slot whose request has
        finished parks -- the attention kernels skip it -- and is refilled with the next request, so a step's work follows the requests
        that are still being answered instead of the longest answer of a fixed group (teochat_amd/stream.py).

        input_ids_list / images_list / stopping_criteria: one entry per request, as generate_batch() takes them; any sequence with
        len() and [] will do -- entry i is read when request i is admitted to a slot, so a lazy sequence keeps only the requests in
        flight in memory.  max_new_tokens: an int or one int per request.  Returns N 1-D tensors prompt + generated in request order,
        each cut at its own stop: greedy, exactly what generate_batch() returns for that request in a group of `slots` conversations.
        Sampling: request i draws from the Philox stream seeded by (the generator's seed, i), so a sampled answer does not depend on
        slots, chunk or the slot the request landed in.  The device stop is armed while every admitted request's stop candidates
        (keyword id lists and EOS, folded as generate() folds them) are one and the same id sequence; otherwise the host applies the
        criteria once per chunk, at the exact token.  `last_generation_stats` = {requests, steps, live_slot_steps, slot_steps,
        prefill_passes} afterwards.

        prefix_keys: one hashable or None per request (any sequence with len() and []) turns prefix reuse on.  Equal keys are the
        caller's promise that the requests' frames are the same; None never shares.  A request whose ids extend what a slot with its
        key already holds -- everything up to and including the last <image>, at least min_prefix_rows embedding rows -- is a HIT: the
        slot's KV rows are copied (teo_kv_fork; not even that when the holder itself is free), only the embeddings of the remaining ids
        are prefilled behind them (teo_llama_prefill_slots_past), the tower does not run and images_list[i] IS NOT READ for it.  Every
        slot keeps a private, complete cache, so the decode step is untouched.  The stats gain prefix_hits, prefix_rows_reused, forks,
        fork_rows, frames_skipped and prefill_rows.  In fp32 the answers are those without keys; in the 16-bit types a prompt prefilled
        in two pieces is not bit for bit the prompt prefilled in one (the suffix's GEMMs and RoPE take the kernels of a short prefill), so
        answers may differ from the keyless run's the way two orderings of a sum differ (prefix reuse).

        share_prefix=True (with prefix_keys only; ValueError otherwise): the decode step reads the rows a slot was forked from ONCE per
        group of slots that hold them instead of once per slot (include/teo_hip_share.h; StreamDecoder.share_prefix).  The private
        copies stay, and the shared step is bit for bit the plain one: the answers are exactly those of share_prefix=False.  The stats
        gain shared_steps (steps that ran the shared form: only while a live slot shares at least one whole key chunk with its
        leader) and shared_rows_skipped (cache rows those steps did not read, per layer and K / V operand).

        guides: one teochat_amd.guide.TokenGuide or None per request (any sequence with len() and []) turns guided decoding on.  The
        distinct guides (by identity) are concatenated into one GuideSet whose table is uploaded once; None is the automaton that allows
        everything.  A request's first token is selected from its prefill logits under its guide's start state, its slot then starts
        from the successor; the step's tail masks, selects and moves every live slot's state (include/teo_hip_guide.h).  EOS stays the
        stop, the guide decides when it is allowed; max_new_tokens may cut an answer mid-pattern.  The stats gain guide_states and
        guide_table_bytes.

        logprobs=True, top_logprobs=k (0..8): returns per request (ids, logprobs [n_new], top ids [n_new, k] or None, top logprobs or None)
        instead of the ids tensor; the values are generate()'s (log softmax of the row each token was selected from, the masked row under
        a guide), recorded by one more launch behind each stream step, plain, guided or shared (include/teo_hip_logprob.h).

        repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens: generate()'s logit rules, ONE setting for every request
        of the call (as the sampler's); each slot keeps its own seen-flags and history, seeded with its request's ids whenever it is
        refilled, so a request's answer does not depend on the slot it landed in or on that slot's earlier occupant.  One more launch in
        front of each stream step's tail, plain, guided, shared or recorded (include/teo_hip_rules.h).  The banning rules are not combined
        with `guides`.  The stats gain the rules in force."""
        from .decode_host import logprob_rows
        from .stream import request_seed, run_stream
        top_n = check_logprob_args(logprobs, top_logprobs)
        N = len(input_ids_list)
        slots = int(slots)
        if N < 1:
            raise ValueError("generate_stream: no requests")
        if not 1 <= slots <= L.MAX_DECODE_BATCH:
            raise ValueError(f"slots {slots} outside 1..{L.MAX_DECODE_BATCH}")
        if share_prefix and prefix_keys is None:
            raise ValueError("share_prefix needs prefix_keys (only forked rows are known to be shared)")
        rules = check_rule_kwargs(dict(repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                                       min_new_tokens=min_new_tokens, suppress_tokens=suppress_tokens, guides=guides),
                                  vocab=self.engine.cfg.vocab_size)
        if eos_token_id == "config":
            eos_token_id = self._config_eos()
        max_new = [int(max_new_tokens)] * N if isinstance(max_new_tokens, int) else [int(m) for m in max_new_tokens]
        if len(max_new) != N:
            raise ValueError("max_new_tokens must be an int or hold one int per request")
        if stopping_criteria is not None and len(stopping_criteria) != N:
            raise ValueError("stopping_criteria must hold one list per request")
        gc = self.generation_config
        temperature = float(getattr(gc, "temperature", 1.0) or 1.0) if temperature is None else temperature
        top_k = getattr(gc, "top_k", 50) if top_k is None else top_k
        top_p = getattr(gc, "top_p", 1.0) if top_p is None else top_p
        tp = 1.0 if (top_p is None or not do_sample) else float(top_p)
        k = int(top_k or 0) if do_sample else 0
        base_seed = 0
        if do_sample:
            base_seed = generator.initial_seed() if generator is not None else int(torch.randint(0, 2 ** 62, (1,)).item())
        eng = self.engine
        dec = self.stream_decoder(slots, max(max(max_new), 1))
        dec.reset()
        gset = None
        if guides is not None:
            from .guide import GuideSet
            if len(guides) != N:
                raise ValueError("guides must hold one TokenGuide (or None) per request")
            gset = GuideSet([guides[r] for r in range(N)], vocab=eng.cfg.vocab_size,
                            eos=eos_token_id if eos_token_id is not None else self._config_eos())
        dec.set_guide(gset)
        dec.share_prefix(bool(share_prefix))
        if logprobs:
            dec.logprobs_begin(top_n)
        dec.rules_begin(slots, rules, eos_ids=[eos_token_id] if eos_token_id is not None else [])
        first_lp = {}                             # request -> its first token's entry (from the prefill logits)
        ids_of, crits_of = {}, {}                 # the requests in flight (and, for ids, the finished ones: a few integers each)
        dev_stop = {"ids": None, "off": False}    # the device stop: one id sequence shared by every request admitted so far, or off

        def stop_candidates(r):
            cands = [ids for c in crits_of[r] for ids in getattr(c, "keyword_id_lists", []) if ids]
            if eos_token_id is not None:
                cands.append([int(eos_token_id)])
            uniq = []
            for ids in cands:
                ids = [int(t) for t in ids]
                if ids not in uniq:
                    uniq.append(ids)
            return uniq

        def register(reqs, with_frames):
            """ids / criteria / the device stop of the requests being admitted; the ids rows and the flat frame list of `with_frames`"""
            rows, flat = [], []
            for r in reqs:
                ids_of[r] = input_ids_list[r].view(-1)
                crits_of[r] = list(stopping_criteria[r]) if stopping_criteria is not None else []
                if r in with_frames:
                    rows.append(ids_of[r])
                    imgs = images_list[r] if images_list is not None else None
                    if imgs is not None:
                        flat.extend(list(imgs))
                uniq = stop_candidates(r)
                if not dev_stop["off"]:
                    if len(uniq) == 1 and dev_stop["ids"] in (None, uniq[0]):
                        dev_stop["ids"] = uniq[0]
                    else:
                        dev_stop["off"] = True
            dec.configure(None if dev_stop["off"] else dev_stop["ids"], do_sample=do_sample, temperature=temperature, top_k=k, top_p=tp)
            return rows, flat

        def embed_rows(reqs, rows, flat):
            """one multimodal preparation for the round, as generate_batch() does it for a group: the embedded rows per request"""
            B = len(reqs)
            dev_ids = rows[0].device
            width = max(int(ids.numel()) for ids in rows)
            ids_p = torch.zeros(B, width, dtype=torch.long, device=dev_ids)
            mask_p = torch.zeros(B, width, dtype=torch.long, device=dev_ids)
            for b, ids in enumerate(rows):
                ids_p[b, :ids.numel()] = ids
                mask_p[b, :ids.numel()] = 1
            (_, _, new_mask, _, embeds, _) = self.prepare_inputs_labels_for_multimodal(ids_p, None, mask_p, None, None, flat or None)
            if embeds is None:
                embeds, new_mask = self.get_model().embed_tokens(ids_p), mask_p
            seqs = []
            for b, r in enumerate(reqs):
                on = torch.nonzero(new_mask[b].to(torch.bool), as_tuple=False).flatten()
                seqs.append(embeds[b, int(on[0]):int(on[-1]) + 1])
            return seqs

        def first_tokens(reqs, logits, lens, slot_list):
            out = []
            if rules is not None:
                # a refilled slot starts from its request's ids and inherits nothing; the first token takes the rules on its prefill row
                logits = logits.contiguous()
                for b, r in enumerate(reqs):
                    dec.rules_seed(slot_list[b], ids_of[r])
                    dec.rules_first(logits[b], slot_list[b])
            if gset is not None:
                # the first token of a request comes from its prefill logits: masked by its guide's start state, and the slot starts
                # from the successor (a slot's earlier occupant left its own last state behind)
                st0 = torch.tensor([gset.starts[r] for r in reqs], dtype=torch.int32, device=eng.device)
                g0 = eng.guide_struct(gset, st0)
                logits = logits.contiguous()
                eng.guide_mask(logits, g0)
            for b, r in enumerate(reqs):
                seed = request_seed(base_seed, r)
                first = eng.sample(logits[b], temperature, k, seed, 0, top_p=tp) if do_sample else self._argmax(logits[b])
                out.append((first, min(max_new[r] - 1, eng.max_seq - lens[b]), seed))
            if logprobs:
                got = [t.cpu() for t in logprob_rows(eng, logits[:len(reqs)].contiguous(), [f[0] for f in out], top_n)]
                for b, r in enumerate(reqs):
                    first_lp[r] = tuple(t[b:b + 1] for t in got)
            if gset is not None:
                eng.guide_advance([f[0] for f in out], g0)
                dec.set_guide_states(slot_list, st0)
            return out

        def admit_past(items):
            """a round's pass with prefix reuse (teochat_amd/stream.py run_stream): items [(request, slot, p ids, P rows)]"""
            reqs = [it[0] for it in items]
            misses = [it[0] for it in items if it[3] == 0]
            rows, flat = register(reqs, set(misses))
            full = dict(zip(misses, embed_rows(misses, rows, flat))) if misses else {}
            seqs, lens, maps = [], [], []
            for r, slot, p, P in items:
                ids = ids_of[r]
                if P:
                    seq = self.get_model().embed_tokens(ids[p:].view(1, -1))[0]          # text ids only (rule c): no tower, no frames
                    maps.append(None)
                else:
                    seq = full[r]
                    n_img = int((ids < 0).sum())
                    nv = (int(seq.shape[0]) - (int(ids.numel()) - n_img)) // n_img if n_img else 0
                    per = [nv if t < 0 else 1 for t in ids.tolist()]
                    maps.append(per if sum(per) == int(seq.shape[0]) else None)           # None: cut by tokenizer_model_max_length, not shared
                n = P + int(seq.shape[0])
                if n + max_new[r] > eng.max_seq:
                    raise ValueError(f"request {r}: prompt ({n}) + max_new_tokens ({max_new[r]}) exceeds max_seq {eng.max_seq}")
                seqs.append(seq)
                lens.append(n)
            logits = dec.refill_past([it[1] for it in items], seqs, [it[3] for it in items])
            return [f + (maps[b], int(seqs[b].shape[0])) for b, f in enumerate(first_tokens(reqs, logits, lens, [it[1] for it in items]))]

        def admit(reqs, slot_list):
            rows, flat = register(reqs, set(reqs))
            seqs = embed_rows(reqs, rows, flat)
            lens = [int(q.shape[0]) for q in seqs]
            for r, n in zip(reqs, lens):
                if max_new[r] > 0 and n + max_new[r] > eng.max_seq:
                    raise ValueError(f"request {r}: prompt ({n}) + max_new_tokens ({max_new[r]}) exceeds max_seq {eng.max_seq}")
            return first_tokens(reqs, dec.refill(slot_list, seqs), lens, slot_list)

        def host_done(r, toks):
            if eos_token_id is not None and toks[-1] == eos_token_id:
                return True
            if crits_of[r]:
                row = torch.cat([ids_of[r].cpu(), torch.tensor(toks, dtype=torch.long)]).unsqueeze(0)
                return any(bool(c(row, None)) for c in crits_of[r])
            return False

        todo = [r for r in range(N) if max_new[r] > 0]
        step_lp = {}                              # request -> what the recorder holds for its step tokens, read when it finishes
        fin = (lambda i, slot, n: step_lp.__setitem__(todo[i], dec.recorded(slot, n))) if logprobs else None
        if prefix_keys is not None and len(prefix_keys) != N:
            raise ValueError("prefix_keys must hold one key (or None) per request")
        if not todo:
            results, stats = [], None
        elif prefix_keys is None:
            results, stats = run_stream(dec, len(todo), slots, lambda reqs, sl: admit([todo[i] for i in reqs], sl),
                                        lambda i, toks: host_done(todo[i], toks), chunk=chunk, on_finish=fin)
        else:
            results, stats = run_stream(dec, len(todo), slots, None, lambda i, toks: host_done(todo[i], toks), chunk=chunk,
                                        keys=[prefix_keys[r] for r in todo], ids_of=lambda i: input_ids_list[todo[i]].view(-1).tolist(),
                                        admit_past=lambda items: admit_past([(todo[i], s, p, P) for i, s, p, P in items]),
                                        min_prefix_rows=min_prefix_rows, on_finish=fin)
        outs = []
        new_of = {todo[i]: toks for i, toks in enumerate(results)}
        for r in range(N):
            ids = ids_of[r] if r in ids_of else input_ids_list[r].view(-1)
            new = new_of.get(r, [])
            outs.append(torch.cat([ids, torch.tensor(new, dtype=ids.dtype, device=ids.device)]) if new else ids.clone())
        if stats is None:
            stats = dict(requests=0, steps=0, live_slot_steps=0, slot_steps=0, prefill_passes=0)
        stats["requests"] = N
        if gset is not None:
            stats.update(guide_states=int(gset.n_states), guide_table_bytes=int(gset.table_bytes))
        if share_prefix:
            stats.update({k: int(dec.stats()[k]) for k in ("shared_steps", "shared_rows_skipped")})
        if rules is not None:
            stats.update(dec.rules_in_force(), suppress_tokens=len(rules[3]))
        dec.set_guide(None)
        dec.share_prefix(False)
        dec.rules_end()
        self.last_generation_stats = stats
        if logprobs:
            dec.logprobs_end()
            z = torch.zeros(0, top_n)
            res = []
            for r in range(N):
                lp, ids, tlp = first_lp.get(r, (torch.zeros(0), z.to(torch.int64), z))
                if r in step_lp:
                    more = step_lp[r]
                    lp = torch.cat([lp, more[0]])
                    if top_n:
                        ids, tlp = torch.cat([ids, more[1]]), torch.cat([tlp, more[2]])
                res.append((outs[r], lp, ids if top_n else None, tlp if top_n else None))
            return res
        return outs

    def _config_eos(self):
        """GenerationMixin semantics: generation_config.eos_token_id (generation_config.json of the checkpoint, or of model_base
        on the LoRA / projector branches) wins; config.json's eos_token_id is what generation_config is seeded from."""
        eos = getattr(self.generation_config, "eos_token_id", None)
        if eos is None:
            eos = getattr(self.config, "eos_token_id", None)
        if isinstance(eos, (list, tuple)):
            eos = eos[0] if eos else None
        return eos

    def _finish(self, input_ids, new_tokens):
        tail = torch.tensor([new_tokens], dtype=input_ids.dtype, device=input_ids.device)
        return torch.cat([input_ids, tail], dim=1)

    def _argmax(self, logits):
        tok = torch.empty(1, dtype=torch.int64, device=self.engine.device)
        with self.engine.phase() as st:
            lg = logits.contiguous()
            L.check(self.engine.lib.teo_argmax(lg.data_ptr(), tok.data_ptr(), 1, lg.numel(), st), "teo_argmax")
        return int(tok.item())
