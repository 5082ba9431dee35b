"""Shared context prefixes without a GPU: the SlotBatch scheduler's use of them against a stub engine, and the
host-side checks of ``ContextPrefix`` and ``build_prompt``."""
import numpy as np
import pytest

from helpers import STUB_K as K, StubEngine


def handle():
    from csm_mlx.models import CSM, csm_tiny
    return CSM(csm_tiny())                 # a host-side handle: no engine is created without a compute call


def prompt(L=5, fill=0):
    return np.full((L, K + 1), fill, np.int32), np.ones((L, K + 1), bool)


def stub_prefix(model, rows, handle_id=1, fill=7):
    """A ContextPrefix that owns nothing on a GPU (no release callable)."""
    from csm_mlx.prefix import ContextPrefix
    return ContextPrefix(model, handle_id, rows, rows * 64, *prompt(rows, fill))


class PrefixStub(StubEngine):
    """StubEngine with the two prefix calls: a load needs a freshly restarted slot and comes before its prefill;
    a save needs a prefilled slot with that many rows."""

    def __init__(self, model, slots, eos):
        super().__init__(slots, eos)
        self.model = model
        self.held = [0] * slots            # rows the slot's cache holds
        self.saved = 100

    def restart(self, b, seed):
        super().restart(b, seed)
        self.held[b] = 0

    def load_prefix(self, items):
        self.log.append(("load_prefix", tuple(b for b, _ in items), tuple(p.handle for _, p in items)))
        for b, p in items:
            assert self.seed[b] is not None and not self.prompt[b] and self.held[b] == 0, "a load into a slot that is not empty"
            self.held[b] = p.rows

    def prefill(self, items):
        super().prefill(items)
        for b, t, _ in items:
            self.held[b] += t.shape[0]

    def save_prefix(self, b, rows, tokens, mask):
        self.log.append(("save_prefix", b, rows))
        assert self.prompt[b] and 1 <= rows <= self.held[b]
        self.saved += 1
        from csm_mlx.prefix import ContextPrefix
        return ContextPrefix(self.model, self.saved, rows, rows * 64, tokens, mask)


def scheduler(slots, eos=None, chunk=4):
    from csm_mlx.batching import SlotBatch
    from csm_mlx.sampling import Sampler
    model = handle()
    stub = PrefixStub(model, slots, eos or {})
    return SlotBatch(model, slots, sampler=Sampler(0.0, 0), chunk=chunk, _engine=stub), stub, model


def boundaries(log):
    """The calls between two runs, as lists of their kinds and the whole events."""
    out, cur = [], []
    for ev in log + [("run", 0)]:
        if ev[0] == "run":
            out.append(cur)
            cur = []
        elif ev[0] != "read":
            cur.append(ev)
    return out


def test_boundary_order_restart_load_prefill_save():
    batch, stub, model = scheduler(3)
    pa, pb = stub_prefix(model, 20, 1), stub_prefix(model, 30, 2)
    plan = [pa, None, pb, pa, None, pa, pb, None]          # 8 utterances, 3 slots, caps of 4 frames
    keep = {1: 3, 3: 22}                                   # utterance 1 keeps 3 of its own 5 rows, 3 keeps 20 + 2
    tickets = [batch.submit(*prompt(5, i + 1), 4, i, prefix=p, keep_rows=keep.get(i, 0)) for i, p in enumerate(plan)]
    out = dict(batch.run())
    assert sorted(out) == sorted(tickets)
    joined = 0
    for calls in boundaries(stub.log):
        if not calls:
            continue
        kinds = [c[0] for c in calls]
        restarted = [c[1] for c in calls if c[0] == "restart"]
        n_r = sum(k in ("restart", "release") for k in kinds)
        assert all(k in ("restart", "release") for k in kinds[:n_r]) and not any(k in ("restart", "release") for k in kinds[n_r:])
        rest = calls[n_r:]
        if not restarted:
            assert not rest
            continue
        jobs = plan[joined: joined + len(restarted)]       # the queue is first in, first out over the free slots
        want_load = tuple(b for b, p in zip(restarted, jobs) if p is not None)
        want = ([("load_prefix", want_load, tuple(p.handle for p in jobs if p is not None))] if want_load else [])
        want.append(("prefill", tuple(restarted)))
        want += [("save_prefix", b, keep[i]) for i, b in zip(range(joined, joined + len(restarted)), restarted) if i in keep]
        assert rest == want, (rest, want)
        joined += len(restarted)
    assert joined == len(plan)
    # exactly one load per boundary that has a prefix join, none elsewhere
    assert sum(e[0] == "load_prefix" for e in stub.log) == sum(
        any(c[0] == "load_prefix" for c in calls) for calls in boundaries(stub.log))
    # kept(): the saved prefixes stand for the first rows of prefix + suffix
    k1, k3 = batch.kept(tickets[1]), batch.kept(tickets[3])
    assert (k1.rows, k3.rows) == (3, 22)
    assert k1.tokens[0, 0] == 2 and k3.tokens[0, 0] == 7 and k3.tokens[21, 0] == 4      # 20 context rows, then its own
    with pytest.raises(ValueError, match="keep_rows"):
        batch.kept(tickets[0])


def test_kept_before_the_join_and_unknown_ticket():
    batch, stub, model = scheduler(1)
    t0 = batch.submit(*prompt(5), 2, 0, keep_rows=4)
    t1 = batch.submit(*prompt(5), 2, 1)
    with pytest.raises(RuntimeError, match="not joined"):
        batch.kept(t0)
    with pytest.raises(ValueError):
        batch.kept(t1)
    with pytest.raises(ValueError):
        batch.kept(99)
    run = batch.run()
    next(run)
    assert batch.kept(t0).rows == 4
    list(run)


def test_submit_counts_prefix_and_suffix_rows():
    from csm_mlx import _lib
    batch, stub, model = scheduler(2)
    S = model.max_seq_len
    p = stub_prefix(model, S - 20)
    batch.submit(*prompt(5), 14, 0, prefix=p)                             # S - 15 < S - 14
    with pytest.raises(ValueError, match=f"Inputs too long \\({S - 15}\\)"):
        batch.submit(*prompt(5), 15, 0, prefix=p)                         # S - 15 >= S - 15
    batch.submit(*prompt(5), 15, 0)                                       # the same rows without the prefix fit
    with pytest.raises(ValueError, match="keep_rows"):
        batch.submit(*prompt(5), 4, 0, prefix=p, keep_rows=S - 14)        # more than prefix + suffix rows
    with pytest.raises(ValueError, match="at least one row"):
        batch.submit(*prompt(0), 4, 0, prefix=p)
    small = handle()
    small.max_frames = 8
    from csm_mlx.batching import SlotBatch
    from csm_mlx.sampling import Sampler
    b2 = SlotBatch(small, 2, sampler=Sampler(0.0, 0), _engine=PrefixStub(small, 2, {}))
    with pytest.raises(_lib.CsmHipError) as ei:                           # the frame-history check is unchanged
        b2.submit(*prompt(5), 9, 0, prefix=stub_prefix(small, 10))
    assert ei.value.code == _lib.CSM_ERR_STATE
    assert not stub.log                                                   # no engine call from any submit


def test_prefix_of_another_model_or_freed_is_refused():
    from csm_mlx.generation import build_prompt
    batch, stub, model = scheduler(2)
    other = handle()
    foreign = stub_prefix(other, 10)
    with pytest.raises(ValueError, match="another model"):
        batch.submit(*prompt(5), 4, 0, prefix=foreign)
    with pytest.raises(ValueError, match="another model"):
        build_prompt(model, [1, 2, 3], 0, foreign)
    mine = stub_prefix(model, 10)
    mine.free()
    mine.free()                                                           # idempotent
    with pytest.raises(RuntimeError, match="freed"):
        batch.submit(*prompt(5), 4, 0, prefix=mine)
    with pytest.raises(ValueError, match="tokens and mask"):
        from csm_mlx.prefix import ContextPrefix
        ContextPrefix(model, 1, 10, 640, *prompt(9))


def test_release_runs_once():
    from csm_mlx.prefix import ContextPrefix
    model, calls = handle(), []
    p = ContextPrefix(model, 5, 3, 192, *prompt(3), release=calls.append)
    p.free()
    p.free()
    del p
    assert calls == [5]
    q = ContextPrefix(model, 6, 3, 192, *prompt(3), release=calls.append)
    del q                                                                  # garbage collection releases too
    assert calls == [5, 6]


def test_build_prompt_with_a_prefix_is_the_text_rows_alone():
    from csm_mlx.generation import build_prompt
    from csm_mlx.tokenizers import tokenize_text_segment
    model = handle()
    ids = [998, 4, 5, 6, 999]
    t, m = build_prompt(model, ids, 1, stub_prefix(model, 40))
    tt, tm = tokenize_text_segment(ids, 1, model.n_audio_codebooks)
    assert np.array_equal(t, tt) and np.array_equal(m, tm) and t.shape == (5, model.n_audio_codebooks + 1)
    t0, m0 = build_prompt(model, ids, 1, [])                              # the list form is unchanged
    assert np.array_equal(t0, tt) and np.array_equal(m0, tm)


def test_start_counts_prefix_rows_before_any_engine_call():
    """generate_codes_batch's window guard: prefix + prompt rows, raised before a FrameCache exists."""
    from csm_mlx.generation import generate_codes_batch
    from csm_mlx.sampling import Sampler
    model = handle()
    S = model.max_seq_len
    p = stub_prefix(model, S - 20)
    with pytest.raises(ValueError, match=f"Inputs too long \\({S - 15}\\)"):
        generate_codes_batch(model, [prompt(5)], 15, sampler=Sampler(0.0, 0), prefixes=[p])
    with pytest.raises(ValueError, match="one prefix"):
        generate_codes_batch(model, [prompt(5)], 4, sampler=Sampler(0.0, 0), prefixes=[p, p])
    assert model._engine is None
