"""One live handle through a long random walk of single setter calls and frame calls (tests/live_handle_cases.py; PARITY.md "Live
handle"): after every frame call the delivered bytes, the requested taps, the sentinels around the buffers, the encoding and the shapes
equal the CPU references for the settings as they then stand, at tolerance 0.  ``configure`` runs once, at step 0; from there on every
device constant of rip_handle.hpp is kept current by the code that notices a change -- which is what runs here.

RIP_WALK_CASES / RIP_WALK_STEPS raise the number and the length of the walks for a soak (default 16 walks of 40 steps)."""
import ctypes as C
import os

import numpy as np
import pytest

import live_handle_cases as L
from helpers import SENTINEL, device_batch
from raw_image_pipeline_amd import RawImagePipeline
from raw_image_pipeline_amd import pipeline as P
from test_heads_gpu import Dest
from test_wb_degenerate_gpu import check_estimate

pytestmark = pytest.mark.gpu

N_CASES = int(os.environ.get("RIP_WALK_CASES", str(len(L.DEFAULT_SEEDS))))
N_STEPS = int(os.environ.get("RIP_WALK_STEPS", str(L.DEFAULT_STEPS)))
SEEDS = list(L.DEFAULT_SEEDS) + [s for s in range(N_CASES) if s not in L.DEFAULT_SEEDS]


class Mismatch(AssertionError):
    pass


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def same(got, ref, what):
    """got / ref: numpy arrays; shapes (in elements) and every byte."""
    if tuple(got.shape) != tuple(ref.shape):
        raise Mismatch("%s: shape %s, expected %s" % (what, tuple(got.shape), tuple(ref.shape)))
    g, r = as_bytes(got), as_bytes(ref)
    if g.size != r.size:
        raise Mismatch("%s: %d bytes, expected %d" % (what, g.size, r.size))
    bad = int((g != r).sum())
    if bad:
        raise Mismatch("%s: %d of %d bytes differ" % (what, bad, g.size))


def torch_bytes(t):
    import torch
    return t.contiguous().view(torch.uint8).cpu().numpy()


def device_input(call, frame_list):
    """The frames of a call as the uint8 stack apply_device takes: [n, rows, cols(, 3)], 16-bit rows as bytes, packed rows as they are."""
    stack = np.stack(frame_list)
    if stack.dtype == np.uint16:
        stack = stack.view(np.uint8).reshape(stack.shape[0], stack.shape[1], stack.shape[2] * 2)
    return np.ascontiguousarray(stack)


def width_of(call):
    return call["size"][0] if L.input_form(call["kind"])[2] else None


def tap_tensors(pipe, call, n):
    import torch
    w, h = call["size"]
    tr, tc, tcn = pipe.query_taps(h, w, L.input_form(call["kind"])[0], call["kind"])
    shape = (n, tr, tc) if tcn == 1 else (n, tr, tc, tcn)
    return [torch.full(shape, SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(2)]


def check_taps(got, e, what):
    for t, ref, name in zip(got, e.taps, ("debayered", "colour")):
        same(t if isinstance(t, np.ndarray) else t.cpu().numpy(), ref, "%s: the %s tap" % (what, name))


def c_frames(t):
    return C.c_void_p(t.data_ptr()), C.c_size_t(t.stride(1)), C.c_size_t(t.stride(0))


def heads_call(pipe, call, t, dests, taps=(None, None)):
    """rip_apply_device_heads through the C ABI into sentinel-filled destinations; (status, message)."""
    import torch
    w, h = call["size"]
    bufs = (P._HeadBuffer * len(dests))()
    for k, d in enumerate(dests):
        if d is not None:
            bufs[k] = d.head_buffer()
    torch.cuda.synchronize()           # the buffers were filled on torch's stream, the handle may be on another
    d_in, in_step, in_frame = c_frames(t)
    st = pipe._lib.rip_apply_device_heads(pipe._h, d_in, in_step, in_frame, int(t.shape[0]), h, w, L.input_form(call["kind"])[0], call["kind"].encode(), bufs, len(dests),
                                          C.c_void_p(taps[0].data_ptr() if taps[0] is not None else 0), C.c_void_p(taps[1].data_ptr() if taps[1] is not None else 0))
    msg = pipe._lib.rip_last_error(pipe._h).decode(errors="replace")
    torch.cuda.synchronize()
    return st, msg


def check_dest(d, ref, what):
    host, mask = d.host(), d.payload_mask()
    if not (host[~mask] == SENTINEL).all():
        raise Mismatch("%s: %d bytes around the delivered rows were written" % (what, int((host[~mask] != SENTINEL).sum())))
    g, r = host[mask], as_bytes(ref)
    if g.size != r.size:
        raise Mismatch("%s: %d delivered bytes, expected %d" % (what, g.size, r.size))
    bad = int((g != r).sum())
    if bad:
        raise Mismatch("%s: %d of %d bytes differ" % (what, bad, g.size))


def head_info(pipe, call, heads):
    w, h = call["size"]
    infos = pipe._head_queries(heads, h, w, L.input_form(call["kind"])[0], call["kind"])
    # a bgr16 result: six bytes per pixel
    return [None if i is None else ((i[0], i[1], 6) + i[3:] if i[3] == "bgr16" else i) for i in infos]


def run_call(pipe, m, call, e):
    import torch
    kind, frame_list = call["kind"], L.frames(call)
    w, h = call["size"]
    cn = L.input_form(kind)[0]
    width = width_of(call)
    sel = m["selected"]
    entry = call["entry"]
    if entry == "process":
        for j, f in enumerate(frame_list):
            out = pipe.process(f, kind, width=width)
            same(out, e.heads[sel][j], "process frame %d" % j)
            assert pipe.last_encoding == e.encodings[sel], (pipe.last_encoding, e.encodings[sel])
            if e.taps is not None:
                same(pipe.get_dist_debayered_image(), e.taps[0][j], "process frame %d: the debayered tap" % j)
                same(pipe.get_dist_color_image(), e.taps[1][j], "process frame %d: the colour tap" % j)
    elif entry in ("apply_device", "apply_device_strided"):
        stack = device_input(call, frame_list)
        batch = device_batch(stack, call["layout"], np.random.default_rng(call["seed"])) if entry == "apply_device_strided" else None
        t = batch.view if batch is not None else torch.from_numpy(stack).cuda()
        taps = tap_tensors(pipe, call, len(frame_list)) if call["taps"] else (None, None)
        out = pipe.apply_device(t, kind, tap_debayered=taps[0], tap_color=taps[1], width=width)
        torch.cuda.synchronize()
        ref = e.heads[sel]
        shape = tuple(ref.shape[:-1]) + (6,) if ref.dtype == np.uint16 and e.encodings[sel] == "bgr16" else tuple(ref.shape)
        if tuple(out.shape) != shape:
            raise Mismatch("%s: shape %s, expected %s" % (entry, tuple(out.shape), shape))
        same(torch_bytes(out).reshape(-1), as_bytes(ref), entry)
        assert pipe.last_encoding == e.encodings[sel], (pipe.last_encoding, e.encodings[sel])
        if call["taps"]:
            check_taps(taps, e, entry)
        if batch is not None:
            batch.check_padding(entry)
    elif entry == "apply_device_heads":
        t = torch.from_numpy(device_input(call, frame_list)).cuda()
        infos = head_info(pipe, call, call["heads"])
        for k in call["heads"]:
            assert infos[k][3] == e.encodings[k], (k, infos[k], e.encodings[k])
        # the base of a bgr16 buffer is a multiple of its two-byte elements: "elem" would put it one byte in
        layouts = {k: "p16" if infos[k][3] == "bgr16" and call["dest"][k] == "elem" else call["dest"][k] for k in call["heads"]}
        dests = [Dest(infos[k], len(frame_list), layouts[k]) if k in call["heads"] else None for k in range(m["n_heads"])]
        taps = tap_tensors(pipe, call, len(frame_list)) if call["taps"] else (None, None)
        st, msg = heads_call(pipe, call, t, dests, taps)
        assert st == P.RIP_OK, msg
        for k in call["heads"]:
            check_dest(dests[k], e.heads[k], "apply_device_heads head %d (%s)" % (k, call["dest"][k]))
        if call["taps"]:
            check_taps(taps, e, entry)
    elif entry == "apply_heads":
        for j, f in enumerate(frame_list):
            outs = pipe.apply_heads(f, kind, heads=call["heads"], width=width)
            assert [o is not None for o in outs] == [k in call["heads"] for k in range(m["n_heads"])]
            for k in call["heads"]:
                same(outs[k], e.heads[k][j], "apply_heads frame %d head %d" % (j, k))
    else:
        assert entry == "submit_collect"
        tickets = [pipe.submit(f, kind, width=width) for f in frame_list]
        for j, ticket in enumerate(tickets):                    # all of them before the next mutation
            same(pipe.collect(ticket), e.heads[sel][j], "collect frame %d" % j)
            assert pipe.last_encoding == e.encodings[sel], (pipe.last_encoding, e.encodings[sel])
    # the getters that follow
    if "wb_info" in call["after"]:
        n = 1 if entry == "process" else len(frame_list)
        info, track = pipe.get_white_balance_info(n), pipe.get_ccc_track(n)
        mode = L.wb_mode(m, kind)
        for j in range(n):
            est = e.estimates[len(frame_list) - n + j]
            try:
                check_estimate("estimate of frame %d" % j, mode, est, info[j], track[j])
            except AssertionError as err:
                raise Mismatch(str(err))
    if "rect_mask" in call["after"]:
        same(pipe.get_rect_mask(), e.rect_mask, "get_rect_mask")
    if "output_mask" in call["after"]:
        same(pipe.get_output_mask(h, w, cn, kind), e.output_mask, "get_output_mask")


def run_refusal(pipe, m, call):
    """The call through the C ABI: the expected status, the head prefix of the message, an empty launch log, untouched destinations."""
    import torch
    kind, frame_list = call["kind"], L.frames(call)
    w, h = call["size"]
    cn = L.input_form(kind)[0]
    want = call["refusal"]
    n = len(frame_list)
    dummy = (h, w, 12, "bgr8", "native")            # the geometry of a refused frame is not defined: room for any element, 16-byte aligned
    with pipe.launch_log() as log:
        if call["entry"] == "process":
            f = np.ascontiguousarray(frame_list[0])
            out = np.full(h * w * 3 * 4 + 64, SENTINEL, np.uint8)
            r, c, k = C.c_int(), C.c_int(), C.c_int()
            st = pipe._lib.rip_apply(pipe._h, f.ctypes.data_as(C.c_void_p), h, w, cn, C.c_size_t(f.strides[0]), kind.encode(), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes),
                                     C.byref(r), C.byref(c), C.byref(k), None)
            msg = pipe._lib.rip_last_error(pipe._h).decode(errors="replace")
            untouched = bool((out == SENTINEL).all())
        else:
            t = torch.from_numpy(device_input(call, frame_list)).cuda()
            if call["entry"] == "apply_device_heads":
                dests = [Dest(dummy, n, "p16") if k in call["heads"] else None for k in range(m["n_heads"])]
                taps = tap_tensors(pipe, call, n) if call["taps"] else (None, None)
                st, msg = heads_call(pipe, call, t, dests, taps)
            else:
                dests = [Dest(dummy, n, "p16")]
                torch.cuda.synchronize()
                d_in, in_step, in_frame = c_frames(t)
                st = pipe._lib.rip_apply_device(pipe._h, d_in, in_step, in_frame, n, h, w, cn, kind.encode(), C.c_void_p(dests[0].ptr), C.c_size_t(0), C.c_size_t(0), None, None)
                msg = pipe._lib.rip_last_error(pipe._h).decode(errors="replace")
            torch.cuda.synchronize()
            untouched = all((d.host() == SENTINEL).all() for d in dests if d is not None)
    assert st == want["status"], "status %d, expected %d: %s" % (st, want["status"], msg)
    assert msg.startswith(want["prefix"]), "message %r, expected the prefix %r" % (msg, want["prefix"])
    assert not log.records(), "a refused call launched: " + log.text
    assert untouched, "a refused call wrote into its destination"


def run_walk(seed, steps, oracle):
    import torch
    assert torch.cuda.is_available(), "gpu-marked test without a GPU"
    pipe = RawImagePipeline(False, "", "", "", device=0)
    streams = [None, torch.cuda.Stream(), torch.cuda.Stream()]       # the test owns them; index 0 is the null stream
    i, step, faulted = 0, None, None
    try:
        for i, step, m, e in L.Evaluator(oracle).replay(steps):
            if step[0] == "init":
                L.apply_model(pipe, m, streams)
            elif step[0] == "mut":
                L.apply_mutation(pipe, step[1], step[2], streams)
            elif e is None:
                run_refusal(pipe, m, step[1])
            else:
                run_call(pipe, m, step[1], e)
    except P.RipError as err:
        if not isinstance(err, (P.RipAssertError, P.RipIOError)):
            faulted = "device error: %s" % err
        else:
            raise AssertionError("walk %d, step %d %r: the library refused an accepted call: %s\nsteps = %s" % (seed, i, step, err, L.format_steps(steps[:i + 1]))) from None
    except RuntimeError as err:                       # torch's own calls report a faulted device this way
        faulted = "torch: %s" % err
    except (AssertionError, ValueError) as err:
        raise AssertionError("walk %d, step %d %r: %s\nreplay with live_handle_cases.walk_from(steps), steps = %s"
                             % (seed, i, step, err, L.format_steps(steps[:i + 1]))) from None
    finally:
        if faulted is None:
            try:
                torch.cuda.synchronize()
                pipe.set_stream(None)
            except (RuntimeError, P.RipError) as err:
                faulted = "after the walk: %s" % err
    if faulted is not None:                           # nothing more is started on a card that has faulted: the session ends here
        pytest.exit("walk %d, step %d %r: %s\nsteps = %s" % (seed, i, step, faulted, L.format_steps(steps[:i + 1])), returncode=3)


@pytest.mark.parametrize("seed", SEEDS)
def test_walk(rip_lib, oracle, seed):
    run_walk(seed, L.walk(seed, N_STEPS), oracle)
