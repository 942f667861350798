"""Graph capture and reused scratch: every chain of tests/capture_cases.py captured once and replayed over changing inputs in the
same buffers, and run big -> small -> big in buffers sized for the big shape - on an MI355X.

The instance suites call an entry once, eagerly, on buffers they have just built.  What they cannot see is what a call leaves
behind for the next call on the same buffers: a status flag that sticks, a counter that does not rewind, scratch of a larger
call.  include/hsr.h promises more than that: no entry allocates or synchronises on a launch path, every one honours its `stream`
and can be captured in a hipGraph.  A capture in global error mode on a non-default stream checks all three without further
tooling (an allocation or a synchronisation fails the capture; a launch on another stream runs outside the graph and overwrites
the sentinel before any replay).

Per row, small shape:
  1. eager warm-up on set 0, compared with the reference (also takes code-object loads out of the capture);
  2. capture of `launch` on ONE side stream (every graph is a chain): every call returns HSR_OK, the outputs still hold what they
     held, the family's launch record names what the eager call named;
  3. replay (set 0), refill(1), replay, refill(2), replay, replay: outputs sentinel-filled before each; after each the row's bar
     against the reference, bit equality with an eager call on fresh buffers, guard zones; the fourth equals the third;
  4. rows that own scratch or a counter: big, small, big - then small twice more, on other sets - in one set of buffers sized for
     the big shape, re-initialising nothing that include/hsr.h does not name; each bit-equal to fresh buffers and within the bar.
The module sets no environment variable and builds no graph with parallel branches.  Every test prints (pytest -s) the launch
record of its captured chain and, for every bounded (not bit-exact) output of its row, the largest observed error over its bar."""
import ctypes as C

import numpy as np
import pytest

import capture_cases as cc
from gpu_harness import LaunchLog, torch_gpu  # noqa: F401  (torch_gpu: the fixture)
from gpu_harness import lib as _lib

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

_FRESH = {}                     # (row, shape, k) -> results of an eager call on fresh buffers
_LOGS = {}


def _log(row):
    if row.log is None:
        return None
    if row.log not in _LOGS:
        _LOGS[row.log] = cc.SrfLog() if row.log == "srf" else LaunchLog(*row.log)
    return _LOGS[row.log]


def _ok(rcs):
    assert rcs and all(rc == 0 for rc in rcs), (rcs, _lib().hsr_last_error())


def _eager(chain, st, k):
    """refill(k), sentinel, launch, results - with the launch record of the chain."""
    log = _log(chain.row)
    chain.refill(k)
    chain.sentinel()
    if log:
        log.clear()
    _ok(chain.launch(st))
    return chain.results(), (log.read() if log else None)


def _fresh(torch, row, st, shape, k):
    key = (row.name, shape, k)
    if key not in _FRESH:
        _FRESH[key] = _eager(row.build(torch, shape), st, k)[0]
    return _FRESH[key]


def _print(name, worst, record=False, captured=None):
    if record:
        print("capture %s: %s" % (name, captured if captured is not None else "(no launch record in this family)"))
    for key, val in sorted(worst.items()):
        print("capture worst [%s] %s: %.4g" % (name, key, val))


def _same(got, want, what, skip=()):
    """Bit equality of every output; work buffers - raw scratch, whose unwritten bytes depend on their history - are left out."""
    for name in want:
        if name in skip:
            continue
        a, b = np.ascontiguousarray(got[name]).view(np.uint8), np.ascontiguousarray(want[name]).view(np.uint8)
        assert a.shape == b.shape, (what, name)
        bad = a != b
        assert not bad.any(), f"{what}: {name} differs in {int(bad.sum())} of {bad.size} bytes, first at byte {int(np.argmax(bad))}"


@pytest.fixture(scope="module")
def side(torch_gpu):
    s = torch_gpu.cuda.Stream()
    assert s.cuda_stream != 0 and s.cuda_stream != torch_gpu.cuda.default_stream().cuda_stream
    return s


@pytest.mark.parametrize("name", list(cc.ROWS))
def test_capture_and_replay(torch_gpu, side, name):
    torch, row = torch_gpu, cc.ROWS[name]
    shape, log = row.shapes["small"], _log(row)
    st = C.c_void_p(side.cuda_stream)
    with torch.cuda.stream(side):
        chain = row.build(torch, shape)
        scratch, worst = tuple(chain.work), {}
        # 1. eager warm-up
        got, names = _eager(chain, st, 0)
        row.check(got, shape, 0, worst)
        if row.instances(shape) is not None:
            assert names == row.instances(shape), (names, row.instances(shape))
        # 2. capture
        chain.restore()
        chain.sentinel()
        before = chain.snapshot()
        graph = torch.cuda.CUDAGraph()
        if log:
            log.clear()
        rcs, errors = None, [_lib().hsr_last_error()]
        with torch.cuda.graph(graph, stream=side, capture_error_mode="global"):       # ends the capture whatever the body does
            rcs = chain.launch(st)
            errors.append(_lib().hsr_last_error())
        assert rcs and all(rc == 0 for rc in rcs), (rcs, errors)
        captured = log.read() if log else None
        assert captured == names, (captured, names)
        after = chain.snapshot()
        for key in before:
            assert np.array_equal(before[key], after[key]), f"{key} changed between the capture and the first replay: a launch ran outside the graph"
        # 3. replays: set 0, 1, 2, and 2 again without a refill
        last = None
        for n, k in enumerate((0, 1, 2, 2)):
            if n in (1, 2):
                chain.refill(k)
            else:
                chain.restore()                                           # in-place operands only: a replay has consumed them
            chain.sentinel()
            torch.cuda.synchronize()
            graph.replay()
            got = chain.results()
            row.check(got, shape, k, worst)
            _same(got, _fresh(torch, row, st, shape, k), f"replay {n + 1} (set {k}) against an eager call on fresh buffers", skip=scratch)
            if n == 3:
                _same(got, last, "the fourth replay against the third", skip=scratch)
            last = got
        del graph
    _print(name, worst, True, captured)


@pytest.mark.parametrize("name", [n for n, r in cc.ROWS.items() if r.reuse])
def test_small_after_big_in_the_same_buffers(torch_gpu, side, name):
    torch, row = torch_gpu, cc.ROWS[name]
    small, big = row.shapes["small"], row.shapes["big"]
    st = C.c_void_p(side.cuda_stream)
    with torch.cuda.stream(side):
        chain = row.build(torch, big)
        scratch, worst = tuple(chain.work), {}
        for shape, k in ((big, 0), (small, 1), (big, 2), (small, 2), (small, 0)):
            chain.set_shape(shape)
            chain.reinit()
            got, _ = _eager(chain, st, k)
            row.check(got, shape, k, worst)
            _same(got, _fresh(torch, row, st, shape, k), f"{'big' if shape == big else 'small'} shape, set {k}, in reused buffers", skip=scratch)
    _print(name + " reuse", worst)
