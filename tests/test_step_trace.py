"""The launches of HDPissaStep are pinned: tools/step_trace.py's CPU matrix (the three exchanges, Wn 1 / 2 / 4,
float32 / bf16 / mixed models, both merge roundings, clipping on and off, default and one-module buckets,
HDP_DELTA_GROUPED 1 and 0, a two-arena model; per configuration four steps with invalidate_factors() and a moved
W_res in between) against tests/golden/step_trace_cpu.txt: one line per configuration -- name, number of trace
lines, SHA-1 of the trace.

A change that claims "the default path launches what it did" passes this test unchanged.  A change that alters
launches on purpose regenerates the file (python tools/step_trace.py --summary > tests/golden/step_trace_cpu.txt)
and shows the diff of the full traces in its pull request."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "step_trace_cpu.txt")


def test_cpu_trace_equals_golden(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import step_trace
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    res = step_trace.run_matrix("cpu")
    assert not [name for name, _, unnamed in res if unnamed], "a tensor argument lies in no named buffer"
    got = [step_trace.summary_line(name, lines) for name, lines, _ in res]
    assert [g.split()[0] for g in got] == [w.split()[0] for w in want], "the matrix itself changed: regenerate the golden file"
    bad = [(g.split()[0], lines) for g, w, (_, lines, _) in zip(got, want, res) if g != w]
    for name, lines in bad[:8]:
        (tmp_path / (name + ".txt")).write_text("\n".join(["## " + name] + lines) + "\n")
    assert not bad, (
        "%d of %d configurations launch something else than the golden trace, the first: %s.  Their full traces "
        "are in %s; to see what changed, run in a checkout of the other commit\n"
        "  python tools/step_trace.py --only %s | diff - %s"
        % (len(bad), len(got), bad[0][0], tmp_path, bad[0][0], tmp_path / (bad[0][0] + ".txt")))
