"""teochat_amd/decode_host.py without a GPU: the host procedures the engine and the three decoders share, on CPU tensors, a recording fake
library and a fake engine whose phase() is a no-op (its hand-off bookkeeping is TeoEngine's own, borrowed unbound)."""
import contextlib
import ctypes as C
import gc

import pytest
import torch

from teochat_amd import _lib as L
from teochat_amd import decode_host as H
from teochat_amd.engine import TeoEngine


class FakeLib:
    """records the calls the helpers make; everything succeeds"""

    def __init__(self, log):
        self.log = log

    def teo_llama_prefill_workspace_bytes(self, desc, rows):
        return 1000 + rows

    def teo_llama_prefill_workspace_status(self, desc, rows, ws, nbytes, flag, stream):
        self.log.append(("status", rows, nbytes))
        flag._obj.value = 0
        return 0

    def teo_graph_launch(self, graph, n, stream):
        self.log.append(("launch", graph.value, n))
        return 0

    def teo_graph_destroy(self, graph):
        self.log.append(("destroy", graph.value))


class FakeStream:
    cuda_stream = 0

    def __init__(self, log):
        self.log = log

    def synchronize(self):
        self.log.append(("sync",))


class FakeEngine:
    _check_handoffs = TeoEngine._check_handoffs
    _run_handoff_check = TeoEngine._run_handoff_check
    on_options, on_tune = TeoEngine.on_options, TeoEngine.on_tune

    def __init__(self):
        self.log = []
        self.lib, self.stream = FakeLib(self.log), FakeStream(self.log)
        self._phase_depth, self._pending_status = 1, {}
        self._option_hooks, self._tune_hooks = H.HookList(), H.HookList()

    def phase(self):
        return contextlib.nullcontext(C.c_void_p(0))

    def _flush_handoff_checks(self, key=None):
        self.log.append(("flush", key))
        TeoEngine._flush_handoff_checks(self, key)

    def _workspace(self, key, nbytes):
        self.log.append(("workspace", key, nbytes))
        return torch.empty(nbytes, dtype=torch.uint8)


# ---------------------------------------------------------------------- sampler arming
ARM = dict(stop_ids=[7, 9], do_sample=True, temperature=0.7, top_k=40, top_p=0.9)


def _armed_state(extra=()):
    s, ids = L.VerifyState(), torch.zeros(16, dtype=torch.int64)
    assert H.arm_sampler(s, ids, extra=extra, **ARM) is True              # a fresh state is greedy with no stop ids: this changes it
    return s, ids


def test_arm_sampler_equal_arguments_are_unchanged():
    s, ids = _armed_state()
    assert H.arm_sampler(s, ids, **ARM) is False
    assert (s.n_stop_ids, s.do_sample, s.top_k) == (2, 1, 40) and ids[:2].tolist() == [7, 9]
    assert s.temperature == C.c_float(0.7).value and s.top_p == C.c_float(0.9).value


@pytest.mark.parametrize("change", [dict(stop_ids=[7, 9, 11]), dict(stop_ids=None), dict(do_sample=False), dict(top_k=41),
                                    dict(temperature=0.8), dict(top_p=0.95)])
def test_arm_sampler_any_changed_field_is_changed(change):
    s, ids = _armed_state()
    assert H.arm_sampler(s, ids, **{**ARM, **change}) is True
    assert H.arm_sampler(s, ids, **{**ARM, **change}) is False            # and the state now holds the new values


def test_arm_sampler_extra_field():
    s, ids = _armed_state(extra=(("max_new", 64),))
    assert s.max_new == 64
    assert H.arm_sampler(s, ids, extra=(("max_new", 64),), **ARM) is False
    assert H.arm_sampler(s, ids, extra=(("max_new", 65),), **ARM) is True and s.max_new == 65


def test_arm_sampler_compares_in_float32():
    s, ids = _armed_state()
    below = 0.7 * (1 + 2.0 ** -30)                                        # another double, the same float32
    assert below != 0.7 and C.c_float(below).value == C.c_float(0.7).value
    assert H.arm_sampler(s, ids, **{**ARM, "temperature": below}) is False
    assert H.arm_sampler(s, ids, **{**ARM, "top_p": 0.9 * (1 + 2.0 ** -30)}) is False


def test_arm_sampler_keeps_the_last_16_stop_ids():
    s, ids = L.DecodeState(), torch.zeros(16, dtype=torch.int64)
    assert H.arm_sampler(s, ids, list(range(100, 120)), False, 1.0, 0, 1.0) is True
    assert s.n_stop_ids == 16 and ids.tolist() == list(range(104, 120))


def test_alloc_loop_state_shapes_and_pointers():
    class Owner:
        pass
    one, many = Owner(), Owner()
    s1, sb = L.DecodeState(), L.DecodeBatchState()
    H.alloc_loop_state(one, s1, "cpu", 32, (50,))
    H.alloc_loop_state(many, sb, "cpu", 32, (3, 50), rows=3)
    assert [tuple(getattr(one, n).shape) for n in ("d_token", "d_pos", "d_out", "d_count", "d_stop", "d_stop_ids", "d_logits", "d_rng")] \
        == [(1,), (1,), (32,), (1,), (1,), (16,), (50,), (2,)]
    assert [tuple(getattr(many, n).shape) for n in ("d_token", "d_pos", "d_out", "d_count", "d_stop", "d_stop_ids", "d_logits", "d_rng")] \
        == [(3,), (3,), (3, 32), (3,), (3,), (16,), (3, 50), (3, 2)]
    for o, s in ((one, s1), (many, sb)):
        assert [getattr(o, n).dtype for n in ("d_token", "d_pos", "d_out", "d_count", "d_stop", "d_stop_ids", "d_logits", "d_rng")] \
            == [torch.int64, torch.int32, torch.int64, torch.int32, torch.int32, torch.int64, torch.float32, torch.int64]
        assert (s.d_token, s.d_pos, s.d_out_tokens, s.d_out_count) == (o.d_token.data_ptr(), o.d_pos.data_ptr(), o.d_out.data_ptr(), o.d_count.data_ptr())
        assert (s.d_stop, s.d_stop_ids, s.d_logits, s.d_rng) == (o.d_stop.data_ptr(), o.d_stop_ids.data_ptr(), o.d_logits.data_ptr(), o.d_rng.data_ptr())
        assert (s.n_stop_ids, s.do_sample, s.top_k, s.temperature, s.top_p) == (0, 0, 0, 1.0, 1.0)


# ---------------------------------------------------------------------- step graphs
class Graphs(H.StepGraphs):
    def __init__(self, eng):
        H.StepGraphs.__init__(self)
        self.lib, self.log, self.made = eng.lib, eng.log, 0

    def create(self, out):
        self.made += 1
        out._obj.value = 100 + self.made
        self.log.append(("create", out._obj.value))

    def step(self):
        self.log.append(("step",))

    def run(self, eng, key, n, use_graph=True, guided=False):
        del self.log[:]
        self.replay_or_step(eng.stream, key, n, use_graph, self.create, self.step, guided=guided)
        return list(self.log)


def test_step_graphs_capture_replay_recapture_and_drop():
    eng = FakeEngine()
    g = Graphs(eng)
    assert g._graph is None and g._guided_graph is None
    assert g.run(eng, "k1", 3) == [("create", 101), ("launch", 101, 3), ("sync",)]          # the first call captures
    assert g._graph is not None
    assert g.run(eng, "k1", 5) == [("launch", 101, 5), ("sync",)]                           # the same key replays
    assert g.run(eng, "k2", 2) == [("destroy", 101), ("create", 102), ("launch", 102, 2), ("sync",)]      # a new key: destroy, then capture
    assert g.run(eng, "k3", 4, use_graph=False) == [("step",)] * 4                          # plain launches: no drain, the graph is left alone
    assert g._graph.value == 102 and g._graph_ws == "k2"
    assert g.run(eng, "g1", 1, guided=True) == [("create", 103), ("launch", 103, 1), ("sync",)]           # a graph of its own beside the plain one
    assert g.run(eng, "k2", 1) == [("launch", 102, 1), ("sync",)]
    del eng.log[:]
    g._drop_graph()
    assert eng.log == [("destroy", 102), ("destroy", 103)] and g._graph is None and g._guided_graph is None
    g._drop_graph()
    assert len(eng.log) == 2                                                                # nothing left to destroy


def test_step_graphs_are_destroyed_with_their_owner():
    eng = FakeEngine()
    g = Graphs(eng)
    g.run(eng, "k", 1)
    del eng.log[:], g
    gc.collect()
    assert eng.log == [("destroy", 101)]


# ---------------------------------------------------------------------- prefill runner
def test_run_prefill_order_and_deferred_check():
    eng, desc = FakeEngine(), L.LlamaDesc()

    def call(ws, stream):
        eng.log.append(("call", ws.numel(), stream.value))
        return 0

    H.run_prefill(eng, desc, 70, "teo_llama_prefill", call)
    assert eng.log == [("flush", "prefill"), ("workspace", "prefill", 1070), ("call", 1070, None), ("status", 70, 1070)]
    # inside a nested phase the check waits ...
    del eng.log[:]
    eng._phase_depth = 2
    H.run_prefill(eng, desc, 9, "teo_llama_prefill", call)
    assert [e[0] for e in eng.log] == ["flush", "workspace", "call"] and list(eng._pending_status) == ["prefill"]
    # ... for the next flush of that key: the next prefill reads the status of the 9-row pass before its own call re-arms the word
    del eng.log[:]
    H.run_prefill(eng, desc, 33, "teo_llama_prefill_batch", call)
    assert eng.log == [("flush", "prefill"), ("status", 9, 1009), ("workspace", "prefill", 1033), ("call", 1033, None)]
    del eng.log[:]
    eng._flush_handoff_checks("vit")                                                        # another key's flush leaves it pending
    assert eng.log == [("flush", "vit")] and list(eng._pending_status) == ["prefill"]
    eng._flush_handoff_checks()
    assert eng.log[-1] == ("status", 33, 1033) and not eng._pending_status


def test_run_prefill_raises_on_a_timed_out_handoff_and_on_a_failed_call(monkeypatch):
    eng, desc = FakeEngine(), L.LlamaDesc()

    def timed_out(desc, rows, ws, nbytes, flag, stream):
        flag._obj.value = 1
        return 0
    eng.lib.teo_llama_prefill_workspace_status = timed_out
    with pytest.raises(RuntimeError, match="teo_llama_prefill_slots: a stream-K / hybrid GEMM hand-off timed out"):
        H.run_prefill(eng, desc, 5, "teo_llama_prefill_slots", lambda ws, st: 0)
    monkeypatch.setattr(L, "load", lambda: type("NoLib", (), {"teo_last_error": staticmethod(lambda: b"bad argument")}))
    with pytest.raises(L.TeoError, match="teo_llama_prefill_slots_past failed with status 2: bad argument"):
        H.run_prefill(eng, desc, 5, "teo_llama_prefill_slots_past", lambda ws, st: 2)


# ---------------------------------------------------------------------- hooks
class Owner:
    def __init__(self):
        self.seen = []


def test_hooks_follow_their_owner():
    eng = FakeEngine()
    live, dead = Owner(), Owner()
    seen_dead = dead.seen
    eng.on_options(live, lambda o, desc: o.seen.append(desc))
    eng.on_options(dead, lambda o, desc: o.seen.append(desc))
    eng.on_tune(dead, lambda o: o.seen.append("knob"))
    eng._option_hooks.fire("d1")
    eng._tune_hooks.fire()
    assert live.seen == ["d1"] and seen_dead == ["d1", "knob"] and len(eng._option_hooks) == 2
    del dead
    gc.collect()
    eng._option_hooks.fire("d2")
    eng._tune_hooks.fire()
    assert live.seen == ["d1", "d2"] and seen_dead == ["d1", "knob"]                        # the collected owner's hooks are not called ...
    assert len(eng._option_hooks) == 1 and len(eng._tune_hooks) == 0                        # ... and are gone from the lists


def test_hook_registered_twice_is_one_hook():
    eng, o = FakeEngine(), Owner()

    def fn(owner, desc):
        owner.seen.append(desc)
    eng.on_options(o, fn)
    eng.on_options(o, fn)
    eng._option_hooks.fire("d")
    assert len(eng._option_hooks) == 1 and o.seen == ["d"]


def test_sync_desc_options_rule():
    src, row, tiled = L.LlamaDesc(), L.LlamaDesc(), L.LlamaDesc()
    src.prefill_fp8, src.rope_in_attn, src.prefill_w4, src.prefill_w4a8 = 1, 1, 1, 1
    H.sync_desc_options(src, [row], [tiled])
    assert (row.prefill_fp8, row.rope_in_attn, row.prefill_w4, row.prefill_w4a8) == (1, 1, 1, 1)
    assert (tiled.prefill_fp8, tiled.rope_in_attn, tiled.prefill_w4, tiled.prefill_w4a8) == (1, 1, 0, 0)


# ---------------------------------------------------------------------- profiled steps
def test_profile_steps_arithmetic():
    K = len(H.PROF_CLASSES)
    assert TeoEngine.PROF_CLASSES is H.PROF_CLASSES
    canned = [([0.5, 0.25] + [0.0] * (K - 2), [2, 1] + [0] * (K - 2)),
              ([1.5, 0.75] + [0.0] * (K - 2), [2, 1] + [0] * (K - 2)),
              ([1.0, 0.5] + [0.0] * (K - 3) + [0.125], [2, 1] + [0] * (K - 3) + [1])]
    it = iter(canned)

    def step(ms, ct):
        m, c = next(it)
        ms[:], ct[:] = m, c
    got = H.profile_steps(3, step)
    # {class: (launches // steps, total ms / launches * 1e3)}; a class that never launched is left out
    assert got == {H.PROF_CLASSES[0]: (2, 3.0 / 6 * 1e3), H.PROF_CLASSES[1]: (1, 1.5 / 3 * 1e3), H.PROF_CLASSES[-1]: (0, 0.125 * 1e3)}
