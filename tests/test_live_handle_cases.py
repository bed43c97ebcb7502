"""The generator of tests/live_handle_cases.py, not the library: the default walks draw what they claim, every (cache, staling kind)
pair of CACHES has a run fill -> change -> read whose two expectations differ, refusals keep their share, CACHES is closed over
rip_handle.hpp, and every expectation of every default walk can be evaluated on the CPU."""
import collections
import os
import re
import time

import pytest

import live_handle_cases as L

HANDLE_HPP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raw_image_pipeline_amd", "csrc", "rip_handle.hpp")


@pytest.fixture(scope="module")
def walks(rip_lib):
    return {seed: L.walk(seed) for seed in L.DEFAULT_SEEDS}


@pytest.fixture(scope="module")
def evaluated(walks, oracle):
    """seed -> [(step, model, kinds, rows, digest or None)]; the expectation of every accepted call of every default walk, once."""
    t0 = time.time()
    out, calls, frames = {}, 0, 0
    for seed, steps in walks.items():
        notes = L.annotate(steps)
        rows = []
        for (i, step, m, e), (_, _, kinds, touched) in zip(L.Evaluator(oracle).replay(steps), notes):
            rows.append((step, m, kinds, touched, L.digest(e) if e is not None else None))
            if e is not None:
                calls += 1
                frames += len(e.F)
        out[seed] = rows
    print("\nlive handle: %d expectations (%d frames) of %d walks evaluated on the CPU in %.1f s" % (calls, frames, len(walks), time.time() - t0))
    return out


def all_steps(walks):
    return [s for steps in walks.values() for s in steps]


def accepted_calls(walks):
    return [(m, s[1]) for steps in walks.values() for s, m in L.walk_from(steps) if s[0] == "call" and s[1]["refusal"] is None]


def test_steps_are_pure_data_and_replay(walks):
    for seed, steps in walks.items():
        assert steps[0] == ("init",) and len(steps) >= L.DEFAULT_STEPS + 1
        again = eval(L.format_steps(steps), {})          # what a failure message prints
        assert again == steps and [m for _, m in L.walk_from(again)] == [m for _, m in L.walk_from(steps)]
        assert steps == L.walk(seed)
        for a, b in zip(steps, steps[1:]):                # a model swap is followed by a reset, on both sides
            if a[0] == "mut" and a[1] == "set_ccc_model":
                assert b[:2] == ("mut", "reset_white_balance_temporal_consistency")
        for s, m in L.walk_from(steps):
            if s[0] == "mut" and s[1] == "set_ccc_model":
                assert m["wb_method"] == "ccc"           # where the reset arms
        assert sum(s[0] == "mut" and s[1] == "load_camera" and s[2][0] == "plumb_bob" for s in steps) <= 1


def test_the_default_walks_draw_every_kind(walks):
    steps = all_steps(walks)
    muts = collections.Counter(s[1] for s in steps if s[0] == "mut")
    assert not [k for k in L.MUTATION_KINDS if not muts[k]], [k for k in L.MUTATION_KINDS if not muts[k]]
    listed = ("set_white_balance_method", "set_fp_contraction", "set_debayer_method", "set_debayer_16bit_range", "set_rect_mask", "set_flip_angle")
    for setter, (_, values) in [(k, v) for k, v in list(L.SCALAR.items()) + list(L.SPREAD.items()) if k in listed]:
        seen = {s[2][0] if setter in L.SCALAR else tuple(s[2]) for s in steps if s[0] == "mut" and s[1] == setter}
        assert seen >= set(values), (setter, set(values) - seen)
    tun = {s[2] for s in steps if s[0] == "mut" and s[1] == "set_tunable"}
    assert {name for name, _ in tun} == set(L.TUNABLES)
    assert {s[2][0] for s in steps if s[0] == "mut" and s[1] == "set_stream"} == {0, 1, 2}
    assert {s[2][0] for s in steps if s[0] == "mut" and s[1] == "load_camera"} == {"equidistant", "plumb_bob"}
    calls = accepted_calls(walks)
    kinds = {"bayer_*16" if c["kind"] in L.BAYER16 else c["kind"] for _, c in calls}
    assert kinds == set(L.BAYER8 + L.COLOUR + L.PACKED) | {"bayer_*16"}, kinds
    assert {c["entry"] for _, c in calls} == set(L.ENTRIES)
    assert {c["n"] for _, c in calls} == set(L.BATCHES)
    assert {c["size"] for _, c in calls} >= set(L.GEOMETRIES + L.CAM_GEOMETRIES + L.CCC_GEOMETRIES)
    assert {c["layout"] for _, c in calls if c["entry"] == "apply_device_strided"} == set(L.H.LAYOUTS[1:])
    assert any(c["taps"] for _, c in calls) and {a for _, c in calls for a in c["after"]} == {"wb_info", "rect_mask", "output_mask"}
    assert {L.wb_mode(m, c["kind"]) for m, c in calls} == {None, "grey_world", "pca", "simple", "ccc"}
    assert any(L.is_bgr16(m, c["kind"]) for m, c in calls) and any(m["cam"] and m["cam"][0] == "plumb_bob" and L.remapped(m) for m, c in calls)
    heads = [m["heads"][k] for m, c in calls for k in L.delivered_heads(m, c)]
    assert {h.interp for h in heads if L.head_resizes(h)} == set(L.INTERPOLATIONS)
    assert {h.fit for h in heads if h.size != (0, 0)} == set(L.FITS)
    assert {h.format for h in heads} == set(L.FORMATS)
    assert any(len(c["heads"]) > 1 for _, c in calls) and any(0 < len(c["heads"]) < m["n_heads"] for m, c in calls)


def test_reverts_same_value_sets_and_double_mutations_reach_every_cache_row(walks):
    steps = all_steps(walks)
    for name, row in L.CACHES.items():
        setters = {s for s in row.stale + row.keep if not s.startswith("call:")}
        for note in ("revert", "same", "double"):
            assert any(s[0] == "mut" and s[1] in setters and note in s[3] for s in steps), "no %s mutation of %s" % (note, name)
    # a double mutation has no frame call in front of it
    for seq in walks.values():
        for a, b in zip(seq, seq[1:]):
            if b[0] == "mut" and "double" in b[3]:
                assert a[0] == "mut"


def test_every_staling_kind_of_every_cache_has_a_run_with_differing_expectations(evaluated, walks, oracle):
    """fill -> the kind -> read.  For a setter the read's expectation must differ, in at least one byte, from the expectation of the
    same call had the setter never been called (live_handle_cases.expected_without): that is what a handle delivers whose cache did not
    notice the setter, and a stale constant that gives the same bytes proves nothing.  For a call kind (another geometry, a larger
    batch, another estimator on the same buffer) the read -- which may be that call itself, the one that meets the stale cache -- must
    differ from the fill; two calls draw different frames, so for these kinds the condition only pins that the run fill -> kind -> read
    exists in a walk, not that a stale prefix or buffer would show in the bytes (the mutants of EXPERIMENTS.md speak to that)."""
    missing, tried = [], 0
    seeds = list(evaluated)
    for name, row in L.CACHES.items():
        masks = name.startswith("mask")
        for kind in row.stale:
            found = False
            first = L.PAIRS.index((name, kind)) % len(seeds)          # the walk whose directed run is this pair's
            for seed in seeds[first:] + seeds[:first]:
                rows = evaluated[seed]
                fills = [i for i, r in enumerate(rows) if name in r[3] and r[4] is not None]
                for k, r in enumerate(rows):
                    if kind not in r[2]:
                        continue
                    before = [i for i in fills if i < k]
                    after = [i for i in fills if i > k or (i == k and kind.startswith("call:"))]
                    if not before or not after:
                        continue
                    if kind.startswith("call:"):
                        found = any(rows[a][4] != rows[b][4] for a in after[:2] for b in before[-2:])
                    elif rows[k][1] != rows[k - 1][1] or kind == "reset_white_balance_temporal_consistency":      # the setter changed something
                        a = after[0]
                        tried += 1
                        stale = L.expected_without(oracle, walks[seed], k, a)
                        if stale is not None:                         # else: without the setter the library refuses the call: no witness
                            real = L.digest(L.expected_without(oracle, walks[seed], None, a), masks) if masks else rows[a][4]
                            found = L.digest(stale, masks) != real
                    if found:
                        break
                if found:
                    break
            if not found:
                missing.append((name, kind))
    print("\nlive handle: %d runs evaluated without their setter" % tried)
    assert not missing, missing


def test_refusals_keep_their_share_and_every_class_occurs(walks):
    calls = [s[1] for s in all_steps(walks) if s[0] == "call"]
    refused = [c for c in calls if c["refusal"] is not None]
    share = len(refused) / len(calls)
    print("\nlive handle: %d of %d call steps are refusals (%.1f %%)" % (len(refused), len(calls), 100 * share))
    assert 0.05 <= share <= 0.15, share
    assert {c["refusal"]["cls"] for c in refused} >= set(L.REFUSAL_CLASSES), collections.Counter(c["refusal"]["cls"] for c in refused)
    for c in refused:
        assert c["refusal"]["status"] in (L.RIP_ERR_INVALID_ARGUMENT, L.RIP_ERR_ASSERT) and not c["after"]
        if c["entry"] in ("apply_device_heads", "apply_heads") and c["refusal"]["cls"] not in ("bgr16_heads", "bgr16_tap"):
            assert re.match(r"output head \d: $", c["refusal"]["prefix"])
    # every walk goes on after a refusal: the next accepted call proves that the refusal moved nothing
    for steps in walks.values():
        idx = [i for i, s in enumerate(steps) if s[0] == "call" and s[1]["refusal"] is not None]
        assert all(any(t[0] == "call" and t[1]["refusal"] is None for t in steps[i + 1:]) for i in idx[:-1])


def test_the_cache_table_is_closed_over_the_handle():
    """Every *Const member of rip_pipeline and every DevBuf whose clean prefix a comment documents has a row: a cache added later fails
    here until it has one."""
    text = open(HANDLE_HPP).read()
    body = text[text.index("struct rip_pipeline {"):]
    body = body[:body.index("\n};")]
    members = re.findall(r"^\s*rip::api::(\w+Const)\s+(\w+)(\[[^\]]*\])?;", body, re.M)
    assert len(members) >= 9, members
    consts = set(re.findall(r"^struct (\w+Const) \{", text, re.M))
    assert {t for t, _, _ in members} == consts, "a *Const struct without a member of rip_pipeline, or the other way round"
    rows = {name.split(".")[0].split("[")[0]: name for name in L.CACHES}
    for _, member, _ in members:
        assert member in rows, "rip_pipeline::%s has no row in live_handle_cases.CACHES" % member
    comments = "\n".join(re.findall(r"//(.*)", body))
    tracked = set(re.findall(r"(\w+)\.clean_bytes", comments))
    assert tracked >= {"d_stats", "d_hist"}
    for buf in tracked:
        assert re.search(r"\bDevBuf\b[^;]*\b%s\b" % buf, body), buf
        assert buf + ".clean_bytes" in L.CACHES, "the clean prefix of %s has no row in live_handle_cases.CACHES" % buf
    for buf in ("d_mid", "d_mht", "d_fmt", "d_rsz"):
        assert re.search(r"\bDevBuf\b[^;]*\b%s\b" % buf, body) and buf + ".cap" in L.CACHES
    kinds = set(L.MUTATION_KINDS) | {"call:geometry", "call:larger", "call:stats", "call:simple", "call:ccc1", "call:cccN"}
    for name, row in L.CACHES.items():
        assert row.stale and row.keep and set(row.stale + row.keep) <= kinds and not set(row.stale) & set(row.keep), name


def test_every_expectation_of_the_default_walks_evaluates_on_the_cpu(evaluated, walks):
    step, m, _, _, d = next(r for r in evaluated[0] if r[4] is not None)         # the first call of a walk: no ccc state in front of it
    assert L.digest(L.expected(m, step[1], L.frames(step[1]))) == d
    for seed, rows in evaluated.items():
        assert len(rows) == len(walks[seed])
        for step, _, _, _, d in rows:
            assert (d is not None) == (step[0] == "call" and step[1]["refusal"] is None)
