"""Single-example inference driver (mirror of the reference's videollava/eval/inference.py:11-77).

run_inference_single keeps the reference's positional order and defaults; `do_sample` is an extra trailing
keyword (the reference hard-codes do_sample=True, inference.py:67) so parity runs can ask for greedy decoding.
"""
import re
from datetime import datetime

import torch

from .constants import DEFAULT_IMAGE_TOKEN, DEFAULT_VIDEO_TOKEN, IMAGE_TOKEN_INDEX
from .conversation import SeparatorStyle, conv_templates
from .mm_utils import KeywordsStoppingCriteria, tokenizer_image_token


def replace_video_token(prompt, image_paths, prompt_strategy):
    n = len(image_paths)
    if prompt_strategy is None:
        expansion = DEFAULT_IMAGE_TOKEN * n
    elif prompt_strategy == "interleave":
        expansion = "".join(f"Image {k}: {DEFAULT_IMAGE_TOKEN}" for k in range(1, n + 1))
    else:
        raise ValueError(f"Unknown prompt strategy: {prompt_strategy}")
    return prompt.replace(DEFAULT_VIDEO_TOKEN, expansion)


def build_prompt(inp, image_paths, conv_mode="v1", prompt_strategy="interleave", chronological_prefix=True):
    conv = conv_templates[conv_mode].copy()
    conv.append_message(conv.roles[0], inp)
    conv.append_message(conv.roles[1], None)
    prompt = conv.get_prompt()
    if chronological_prefix:
        prompt = prompt.replace("times:", "times in chronological order:")
    stop_str = conv.sep2 if conv.sep_style == SeparatorStyle.TWO else conv.sep
    return replace_video_token(prompt, image_paths, prompt_strategy), stop_str


def run_inference_single(model, processor, tokenizer, inp, image_paths, conv_mode="v1", timestamps=[],
                         prompt_strategy="interleave", chronological_prefix=True, temperature=0.2, max_new_tokens=256,
                         do_sample=True, prompt_lookup_num_tokens=None, max_matching_ngram_size=None, guide=None, repetition_penalty=None,
                         no_repeat_ngram_size=None, num_beams=None, return_logprobs=False):
    """guide (extra trailing keyword): a teochat_amd.guide.TokenGuide over the tokenizer's vocabulary -- the answer is generated under it
    (model.generate(guide=...)); None: the keyword is not passed on.
    return_logprobs=True (extra trailing keyword): returns (text, {"logprobs": [...], "confidence": float, "box_confidences": [...]}) --
    model.generate(logprobs=True) and teochat_amd/confidence.py over the generated tokens, the stop token included.
    repetition_penalty / no_repeat_ngram_size (extra trailing keywords): model.generate's logit rules (include/teo_hip_rules.h); None: the
    keyword is not passed on.
    num_beams (extra keyword in front of return_logprobs): model.generate's beam search (include/teo_hip_beam.h); above 1 it forces do_sample=False, None:
    the keyword is not passed on."""
    if len(timestamps) > 0:
        order = sorted(range(len(image_paths)), key=lambda i: datetime.strptime(timestamps[i], "%Y-%m-%d"))
        image_paths = [image_paths[i] for i in order]
        timestamps = [timestamps[i] for i in order]
    frames = [processor.preprocess(p, return_tensors="pt")["pixel_values"][0] for p in image_paths]
    frames = [f.to(model.device, dtype=model.dtype) for f in frames]
    prompt, stop_str = build_prompt(inp, image_paths, conv_mode, prompt_strategy, chronological_prefix)
    input_ids = tokenizer_image_token(prompt, tokenizer, IMAGE_TOKEN_INDEX, return_tensors="pt").unsqueeze(0).to(model.device)
    stopping = KeywordsStoppingCriteria([stop_str], tokenizer, input_ids)
    with torch.inference_mode():
        spec = {}                                  # prompt-lookup speculative decoding (model.generate): passed on only when asked for
        if prompt_lookup_num_tokens is not None:
            spec["prompt_lookup_num_tokens"] = prompt_lookup_num_tokens
        if max_matching_ngram_size is not None:
            spec["max_matching_ngram_size"] = max_matching_ngram_size
        if guide is not None:
            spec["guide"] = guide
        if return_logprobs:
            spec["logprobs"] = True
        if repetition_penalty is not None:
            spec["repetition_penalty"] = repetition_penalty
        if no_repeat_ngram_size is not None:
            spec["no_repeat_ngram_size"] = no_repeat_ngram_size
        if num_beams is not None:
            spec["num_beams"] = num_beams
            if int(num_beams) > 1:
                do_sample = False
        output_ids = model.generate(input_ids=input_ids, images=frames, do_sample=do_sample, temperature=temperature,
                                    max_new_tokens=max_new_tokens, use_cache=True, stopping_criteria=[stopping], **spec)
    if return_logprobs:
        new = output_ids.sequences[0, input_ids.shape[1]:]
        return _text(tokenizer, new), _confidence(model, tokenizer, new, output_ids.logprobs[0])
    return tokenizer.decode(output_ids[0, input_ids.shape[1]:]).replace("</s>", "").strip()


def _text(tokenizer, new_ids):
    return tokenizer.decode(new_ids).replace("</s>", "").strip()


def _confidence(model, tokenizer, new_ids, logprobs):
    """confidence.confidence_record of one answer; the tokenizer's pieces are computed once per (model, tokenizer)"""
    from .confidence import confidence_record
    from .guide import pieces_of
    cached = getattr(model, "_pieces_cache", None)
    if cached is None or cached[0] is not tokenizer:
        cached = (tokenizer, pieces_of(tokenizer, vocab=getattr(getattr(model, "config", None), "vocab_size", None)))
        try:
            model._pieces_cache = cached
        except AttributeError:
            pass
    n = int(new_ids.numel())
    return confidence_record(cached[1], new_ids, logprobs[:n])


def option_token_ids(tokenizer, option):
    """The ids an answer option is scored on: the tokenizer's ids without the leading BOS, followed by EOS -- the reference's answer
    followed by `</s>`, so that "Airport" is not favoured over "Airport Hangar" for being its prefix."""
    ids = [int(t) for t in tokenizer(option).input_ids]
    bos = getattr(tokenizer, "bos_token_id", None)
    if ids and bos is not None and ids[0] == bos:
        ids = ids[1:]
    return ids + [int(tokenizer.eos_token_id)]


def run_inference_options(model, processor, tokenizer, inp, image_paths, options, conv_mode="v1", timestamps=[],
                          prompt_strategy="interleave", chronological_prefix=True, normalize=False):
    """Closed-set answer: scores log p(option + </s> | frames, question) of every option (model.score_options: all options in one
    pass over the weights) and returns (best option, fp32 scores [N] on the CPU).  The prompt is run_inference_single's.
    normalize=True divides every score by its option's token count before the argmax (the returned scores are the divided ones)."""
    options = list(options)
    if not options:
        raise ValueError("run_inference_options: no options")
    if len(timestamps) > 0:
        order = sorted(range(len(image_paths)), key=lambda i: datetime.strptime(timestamps[i], "%Y-%m-%d"))
        image_paths = [image_paths[i] for i in order]
        timestamps = [timestamps[i] for i in order]
    frames = [processor.preprocess(p, return_tensors="pt")["pixel_values"][0] for p in image_paths]
    frames = [f.to(model.device, dtype=model.dtype) for f in frames]
    prompt, _ = build_prompt(inp, image_paths, conv_mode, prompt_strategy, chronological_prefix)
    input_ids = tokenizer_image_token(prompt, tokenizer, IMAGE_TOKEN_INDEX, return_tensors="pt").unsqueeze(0).to(model.device)
    option_ids = [option_token_ids(tokenizer, o) for o in options]
    with torch.inference_mode():
        scores = model.score_options(input_ids, frames, option_ids).detach().float().cpu()
    if normalize:
        scores = scores / torch.tensor([float(len(ids)) for ids in option_ids])
    return options[int(scores.argmax())], scores


def run_inference_batch(model, processor, tokenizer, inps, image_paths_list, conv_mode="v1", timestamps_list=None,
                        prompt_strategy="interleave", chronological_prefix=True, temperature=0.2, max_new_tokens=256,
                        do_sample=True, continuous=False, slots=None, prefix_cache=False, guides=None, share_prefix=False, logprobs=False,
                        repetition_penalty=None, no_repeat_ngram_size=None):
    """run_inference_single for up to 16 examples at once (not in the reference, whose loop is one example at a time,
    inference.py:100-113): the same prompt construction, frame order, tokenisation and stop keyword per example, then ONE
    batched generation -- every frame of every example through the tower together, one prefill per example, and a decode loop
    that streams each weight matrix once per step for all examples (LlavaLlamaForCausalLM.generate_batch).  Greedy decoding
    gives the single-example answers; sampling draws from per-example Philox streams seeded from torch's global generator,
    so a sampled run is reproducible under torch.manual_seed but is not the single-example loop's stream.

    continuous=True (extra trailing keyword): ANY number of examples through one LlavaLlamaForCausalLM.generate_stream over
    `slots` (default min(number of examples, 16)) conversation slots -- a slot whose answer has finished is refilled with the next
    example instead of idling until the longest answer of its group ends.  The same prompts, frames and stop keywords, each
    prepared when its example is admitted to a slot (inps, image_paths_list and timestamps_list may be lazy sequences); greedy
    answers equal the static path's, sampled ones draw from per-EXAMPLE Philox streams.

    prefix_cache=True (with continuous=True only): examples about the same image sequence share its prefill -- generate_stream's
    prefix_keys, the key being the tuple of the example's image paths after the timestamp sort (paths that are not strings: no key).
    An example that starts from another one's rows neither opens nor preprocesses its images.

    guides (with continuous=True only): one teochat_amd.guide.TokenGuide or None per example (any sequence with len() and []), handed to
    generate_stream(guides=...).

    share_prefix=True (with prefix_cache=True only): generate_stream(share_prefix=True) -- the decode step reads the rows examples were
    forked from once per group of slots; the answers are the same.

    logprobs=True: every entry of the returned list is (text, confidence record) as run_inference_single(return_logprobs=True) returns
    them (generate_batch / generate_stream with logprobs=True).

    repetition_penalty / no_repeat_ngram_size (with continuous=True only): generate_stream's logit rules, one setting for all examples."""
    B = len(inps)
    rule_kw = {k: v for k, v in (("repetition_penalty", repetition_penalty), ("no_repeat_ngram_size", no_repeat_ngram_size)) if v is not None}
    if rule_kw and not continuous:
        raise ValueError("repetition_penalty / no_repeat_ngram_size need continuous=True (generate_stream applies the rules per slot; the "
                         "fixed-group batched step has no form with them)")
    if share_prefix and not prefix_cache:
        raise ValueError("share_prefix needs prefix_cache=True (only forked rows are known to be shared)")
    if prefix_cache and not continuous:
        raise ValueError("prefix_cache needs continuous=True (prefix reuse lives in the stream decoder's slots)")
    if guides is not None and not continuous:
        raise ValueError("guides needs continuous=True (generate_stream takes one guide per request; the fixed-group batched step takes none)")
    if continuous:
        return _run_inference_stream(model, processor, tokenizer, inps, image_paths_list, conv_mode, timestamps_list, prompt_strategy,
                                     chronological_prefix, temperature, max_new_tokens, do_sample, slots, prefix_cache, guides, share_prefix,
                                     logprobs, rule_kw)
    if timestamps_list is None:
        timestamps_list = [[] for _ in range(B)]
    if len(image_paths_list) != B or len(timestamps_list) != B:
        raise ValueError("run_inference_batch: one image list and one timestamp list per question")
    ids_list, frames_list, crits, n_prompt = [], [], [], []
    for inp, image_paths, timestamps in zip(inps, image_paths_list, timestamps_list):
        if len(timestamps) > 0:
            order = sorted(range(len(image_paths)), key=lambda i: datetime.strptime(timestamps[i], "%Y-%m-%d"))
            image_paths = [image_paths[i] for i in order]
        frames = [processor.preprocess(p, return_tensors="pt")["pixel_values"][0] for p in image_paths]
        frames_list.append([f.to(model.device, dtype=model.dtype) for f in frames])
        prompt, stop_str = build_prompt(inp, image_paths, conv_mode, prompt_strategy, chronological_prefix)
        input_ids = tokenizer_image_token(prompt, tokenizer, IMAGE_TOKEN_INDEX, return_tensors="pt").unsqueeze(0).to(model.device)
        ids_list.append(input_ids[0])
        n_prompt.append(input_ids.shape[1])
        crits.append([KeywordsStoppingCriteria([stop_str], tokenizer, input_ids)])
    with torch.inference_mode():
        outs = model.generate_batch(ids_list, frames_list, do_sample=do_sample, temperature=temperature,
                                    max_new_tokens=max_new_tokens, stopping_criteria=crits, **({"logprobs": True} if logprobs else {}))
    if logprobs:
        return [(_text(tokenizer, o[0][n:]), _confidence(model, tokenizer, o[0][n:], o[1])) for o, n in zip(outs, n_prompt)]
    return [tokenizer.decode(o[n:]).replace("</s>", "").strip() for o, n in zip(outs, n_prompt)]


class _Prepared:
    """Example i's (input ids, frames, criteria), built when first asked for; the last `keep` examples are kept, so that the ids, the
    frames and the criteria of one example come from one preparation while no more than a lookahead of them is held.  A column in `lazy`
    holds a function until it is indexed for the first time (the frames: an example that reuses a prefix never opens its images)."""

    def __init__(self, prepare, n, keep, lazy=()):
        self.prepare, self.n, self.keep, self.cache, self.lazy = prepare, n, keep, {}, tuple(lazy)

    def get(self, i):
        if i not in self.cache:
            self.cache[i] = self.prepare(i)
            for j in list(self.cache)[:-self.keep]:          # insertion order: the oldest preparations go
                del self.cache[j]
        return self.cache[i]

    def column(self, k):
        outer = self

        class Column:
            def __len__(self):
                return outer.n

            def __getitem__(self, i):
                row = outer.get(i)
                if k in outer.lazy and callable(row[k]):
                    row[k] = row[k]()
                return row[k]
        return Column()


def _run_inference_stream(model, processor, tokenizer, inps, image_paths_list, conv_mode, timestamps_list, prompt_strategy,
                          chronological_prefix, temperature, max_new_tokens, do_sample, slots, prefix_cache=False, guides=None,
                          share_prefix=False, logprobs=False, rule_kw=None):
    N = len(inps)
    if N == 0:
        return []
    if len(image_paths_list) != N or (timestamps_list is not None and len(timestamps_list) != N):
        raise ValueError("run_inference_batch: one image list and one timestamp list per question")
    slots = min(N, 16) if slots is None else int(slots)
    n_prompt = {}

    def sorted_paths(i):
        image_paths = image_paths_list[i]
        timestamps = timestamps_list[i] if timestamps_list is not None else []
        if len(timestamps) > 0:
            order = sorted(range(len(image_paths)), key=lambda k: datetime.strptime(timestamps[k], "%Y-%m-%d"))
            image_paths = [image_paths[k] for k in order]
        return image_paths

    def prepare(i):
        image_paths = sorted_paths(i)

        def frames():
            return [processor.preprocess(p, return_tensors="pt")["pixel_values"][0].to(model.device, dtype=model.dtype) for p in image_paths]
        prompt, stop_str = build_prompt(inps[i], image_paths, conv_mode, prompt_strategy, chronological_prefix)
        input_ids = tokenizer_image_token(prompt, tokenizer, IMAGE_TOKEN_INDEX, return_tensors="pt").unsqueeze(0).to(model.device)
        n_prompt[i] = input_ids.shape[1]
        return [input_ids[0], frames, [KeywordsStoppingCriteria([stop_str], tokenizer, input_ids)]]

    class Keys:
        """the prefix key of example i: its image paths after the timestamp sort (None when a path is not a string)"""

        def __len__(self):
            return N

        def __getitem__(self, i):
            paths = list(sorted_paths(i))
            return tuple(paths) if paths and all(isinstance(p, str) for p in paths) else None

    prepared = _Prepared(prepare, N, 2 * slots, lazy=(1,))
    with torch.inference_mode():
        outs = model.generate_stream(prepared.column(0), prepared.column(1), slots=slots, do_sample=do_sample, temperature=temperature,
                                     max_new_tokens=max_new_tokens, stopping_criteria=prepared.column(2),
                                     **({"prefix_keys": Keys()} if prefix_cache else {}), **({"guides": guides} if guides is not None else {}),
                                     **({"share_prefix": True} if share_prefix else {}), **({"logprobs": True} if logprobs else {}),
                                     **(rule_kw or {}))
    if logprobs:
        return [(_text(tokenizer, o[0][n_prompt[i]:]), _confidence(model, tokenizer, o[0][n_prompt[i]:], o[1])) for i, o in enumerate(outs)]
    return [tokenizer.decode(o[n_prompt[i]:]).replace("</s>", "").strip() for i, o in enumerate(outs)]


_BBOX = re.compile(r"\[(\d+), (\d+), (\d+), (\d+)\]")
_POLYGON_DATASETS = ["xbd_loc", "xbd_dmg_cls", "s2_det", "qfabric_rqa2", "qfabric_rqa5", "xbd_sre_qa_rqa", "s2_sre_qa", "s2_rqa"]


def extract_bboxes(bbox_str):
    """'[x1, y1, x2, y2]' groups of integers (exactly ', '-separated) -> [[x1, y1, x2, y2], ...]  (inference.py:80-85)."""
    return [[int(v) for v in m.groups()] for m in _BBOX.finditer(bbox_str)]


def _record(example, response, dataset):
    question, answer = example["conversations"][0]["value"], example["conversations"][1]["value"]
    record = {"response": response, "ground_truth": answer, "task": example["task"]}
    polygon = example.get("polygon", None)
    if polygon is not None:
        record["polygon"] = polygon
    elif dataset in _POLYGON_DATASETS:            # as in the reference: only a dataset passed by NAME can trip this
        raise ValueError(f"Polygons not found for dataset {dataset}. The TEOChatlas dataset was updated to include these "
                         "polygons on 25 Mar 2025. Please re-download the json files for these splits.")
    boxes_in, boxes_out = extract_bboxes(question), extract_bboxes(answer)
    if boxes_in:
        record["input_bboxes"] = boxes_in
    if boxes_out:
        record["output_bboxes"] = boxes_out
    return record


def run_inference(dataset, model, tokenizer, processor, prompt_strategy, chronological_prefix, conv_mode, temperature,
                  max_new_tokens, batch_size=1, continuous=False, prefix_cache=False, guide=None, share_prefix=False, logprobs=False,
                  repetition_penalty=None, no_repeat_ngram_size=None, num_beams=None):
    """Dataset loop with the bookkeeping the metrics need (inference.py:88-137): response / ground truth / task per example,
    the example's polygon when it has one, and the integer boxes quoted in the question and in the reference answer.
    batch_size (extra trailing keyword, default 1 = the reference's loop): answer that many consecutive examples per
    generation (run_inference_batch, <= 16); the records come out in dataset order either way.
    continuous=True (extra trailing keyword, default off): the whole dataset goes through ONE generate_stream over batch_size
    conversation slots (run_inference_batch(continuous=True)); examples are read and prepared as slots free up.
    prefix_cache=True (with continuous=True): examples with the same image paths share the prefill of everything up to their last
    <image> (run_inference_batch(prefix_cache=True)); the records are the same.
    share_prefix=True (with continuous=True and prefix_cache=True): the decode step reads the rows examples were forked from once per
    group of slots (run_inference_batch(share_prefix=True)); the records are the same.
    guide (extra trailing keyword): a teochat_amd.guide.TokenGuide for every example, or a callable(example) -> TokenGuide or None.  With
    batch_size 1 it goes to run_inference_single(guide=...), with continuous=True to generate_stream(guides=...); groups of a fixed
    batch_size > 1 take no guide (ValueError).
    logprobs=True (extra trailing keyword): every record gains `confidence` (exp of the mean token log-probability of the answer) and
    `box_confidences` ([[box, score], ...] for the boxes of the response; teochat_amd/confidence.py), at batch_size 1, in groups and
    continuous alike.  The metrics functions do not read the two keys.
    repetition_penalty / no_repeat_ngram_size (extra trailing keywords): the logit rules of generate() (batch_size 1) or of
    generate_stream() (continuous=True); groups of a fixed batch_size > 1 take none (ValueError).
    num_beams (extra trailing keyword): beam search of generate() (include/teo_hip_beam.h), batch_size 1 without continuous only."""
    if num_beams is not None and int(num_beams) > 1 and (continuous or batch_size != 1):
        raise ValueError("num_beams needs batch_size=1 without continuous (beam search runs one conversation over the batched step's slots)")
    lp_kw = {"logprobs": True} if logprobs else {}
    rule_kw = {k: v for k, v in (("repetition_penalty", repetition_penalty), ("no_repeat_ngram_size", no_repeat_ngram_size)) if v is not None}
    if rule_kw and not continuous and batch_size != 1:
        raise ValueError("repetition_penalty / no_repeat_ngram_size need batch_size=1 or continuous=True")

    def record(example, response):
        if not logprobs:
            return _record(example, response, dataset)
        rec = _record(example, response[0], dataset)
        rec["confidence"], rec["box_confidences"] = response[1]["confidence"], response[1]["box_confidences"]
        return rec
    if not 1 <= int(batch_size) <= 16:
        raise ValueError(f"batch_size {batch_size}: 1..16 examples per generation")
    if prefix_cache and not continuous:
        raise ValueError("prefix_cache needs continuous=True")
    if share_prefix and not prefix_cache:
        raise ValueError("share_prefix needs prefix_cache=True")
    if guide is not None and not continuous and batch_size != 1:
        raise ValueError("guide needs batch_size=1 or continuous=True")
    guide_of = guide if callable(guide) else (lambda example: guide)
    outputs = []
    if continuous:
        n = len(dataset)

        class Field:
            def __init__(self, get):
                self.get = get

            def __len__(self):
                return n

            def __getitem__(self, i):
                return self.get(dataset[i])
        responses = run_inference_batch(model, processor, tokenizer, Field(lambda e: e["conversations"][0]["value"]),
                                        Field(lambda e: e["video"]), conv_mode=conv_mode, timestamps_list=Field(lambda e: e["timestamp"]),
                                        prompt_strategy=prompt_strategy, chronological_prefix=chronological_prefix, temperature=temperature,
                                        max_new_tokens=max_new_tokens, continuous=True, slots=int(batch_size),
                                        **({"prefix_cache": True} if prefix_cache else {}),
                                        **({"share_prefix": True} if share_prefix else {}),
                                        **({"guides": Field(guide_of)} if guide is not None else {}), **lp_kw, **rule_kw)
        return [record(dataset[i], r) for i, r in enumerate(responses)]
    if batch_size == 1:
        for example in dataset:
            response = run_inference_single(model, processor, tokenizer, example["conversations"][0]["value"], example["video"],
                                            conv_mode=conv_mode, timestamps=example["timestamp"], prompt_strategy=prompt_strategy,
                                            chronological_prefix=chronological_prefix, temperature=temperature,
                                            max_new_tokens=max_new_tokens, **({"guide": guide_of(example)} if guide is not None else {}),
                                            **({"return_logprobs": True} if logprobs else {}), **rule_kw,
                                            **({"num_beams": num_beams} if num_beams is not None else {}))
            outputs.append(record(example, response))
        return outputs
    group = []

    def flush():
        if not group:
            return
        responses = run_inference_batch(model, processor, tokenizer, [e["conversations"][0]["value"] for e in group],
                                        [e["video"] for e in group], conv_mode=conv_mode,
                                        timestamps_list=[e["timestamp"] for e in group], prompt_strategy=prompt_strategy,
                                        chronological_prefix=chronological_prefix, temperature=temperature,
                                        max_new_tokens=max_new_tokens, **lp_kw)
        outputs.extend(record(e, r) for e, r in zip(group, responses))
        group.clear()

    for example in dataset:
        group.append(example)
        if len(group) == batch_size:
            flush()
    flush()
    return outputs
