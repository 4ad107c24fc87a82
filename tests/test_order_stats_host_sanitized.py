"""The cost-ordered dispatch (csrc/ptmi_order.cpp), the statistics and the option table under AddressSanitizer + UndefinedBehaviorSanitizer,
without a GPU: a stand-alone program (tests/cxx/order_stats_hostsan.cpp, its own main) linked statically against the sanitizer's runtime,
against the HIP stand-in and against the library with instrumented host code, and run directly -- nothing is preloaded, nothing is loaded
into Python (tests/test_chain_stream_host_sanitized.py builds and runs it).

`plain`: after every ABI call of one fixed scenario what the call did to the runtime, which launches were handed the order and the cost
words, what the order kernel was given for the tail, and every option's accepted and refused values with their messages.
tests/golden/order_stats_calls.txt is that record of the commit before the order, the statistics and the options got an owner each: the
same runtime calls, codes and messages, line for line.  `walk`: every runtime call of a context's creation, launches 0 to 4 at 64x16 and
the statistics calls fails in turn; every failure leaves a context that renders again and is destroyed clean."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_host_sanitized as hs  # noqa: E402
import test_chain_stream_host_sanitized as cs  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "order_stats_calls.txt")


@hs.needs_asan
def test_the_order_the_statistics_and_the_options_make_the_recorded_runtime_calls_and_survive_every_failure():
    program = cs.build_program(program="order_stats_hostsan")
    got = cs.run_program(program, "plain").splitlines()
    with open(GOLDEN) as fh:
        want = fh.read().splitlines()
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, "line %d: %r, recorded %r" % (i + 1, a, b)
    assert len(got) == len(want), "%d lines, %d recorded" % (len(got), len(want))
    # the walk fails every runtime call in turn: at least as many failure points as the record counts calls (the six numbers after `calls`)
    # for the steps it walks
    calls = lambda line: sum(int(v) for v in line.split(" calls ")[1].split(" live ")[0].split())      # noqa: E731
    floor = sum(calls(line) for line in want if line.startswith("walked: "))
    walked = cs.run_program(program, "walk")
    points = int(re.search(r"walk: (\d+) failure points", walked).group(1))
    assert floor >= 40 and points >= floor, (points, floor)
