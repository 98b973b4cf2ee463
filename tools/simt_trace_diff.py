#!/usr/bin/env python3
"""Compare two SIMT_EMU_TRACE logs of the CPU stand-in (tests/cpp/simt_emu), stream by stream.

    SIMT_EMU_TRACE=1 <a run against build A> 2> a.trace ;  the same against build B 2> b.trace
    tools/simt_trace_diff.py a.trace b.trace

The stand-in runs every launch synchronously and ignores streams and events, so a refactor of the host code that moves a launch to
another stream, or a wait in front of the record it waits for, passes every parity test on it.  The trace has one line per launch
(kernel, grid, block, stream), event record, stream wait and synchronise, with streams and events numbered in creation order.  The
worker thread makes the global interleaving unstable, so the durations are dropped and each trace is projected per stream (event
synchronises, which belong to no stream: "host"); the projections are diffed.  Every wait whose event has no earlier record in host
order is listed as well, for both traces.  Exit status 0: projections and lists are identical."""
import difflib
import re
import sys

PAT = [(re.compile(r"^.* <<<.*>>> stream (\d+)$"), 1), (re.compile(r"^record event \d+ stream (\d+)$"), 1),
       (re.compile(r"^wait stream (\d+) event (\d+)$"), 1), (re.compile(r"^sync stream (\d+)$"), 1)]


def load(path):
    """({stream: [lines]}, [waits without an earlier record], number of trace lines)"""
    streams, recorded, unrecorded, n = {}, set(), [], 0
    for raw in open(path, errors="replace"):
        if not raw.startswith("[simt_emu] "):
            continue
        n += 1
        line = re.sub(r" [0-9.]+ ms$", "", raw[len("[simt_emu] "):].rstrip("\n"))
        key = "host"
        for pat, grp in PAT:
            m = pat.match(line)
            if m:
                key = m.group(grp)
                break
        own = streams.setdefault(key, [])
        if line.startswith("record event "):
            recorded.add(line.split()[2])
        elif line.startswith("wait stream ") and line.split()[4] not in recorded:
            unrecorded.append("%s (entry %d of stream %s)" % (line, len(own), key))
        own.append(line)
    return streams, unrecorded, n


def main(a, b):
    (sa, ua, na), (sb, ub, nb) = load(a), load(b)
    same = True
    for key in sorted(set(sa) | set(sb), key=lambda k: (k == "host", k.zfill(4))):
        la, lb = sa.get(key, []), sb.get(key, [])
        if la == lb:
            print("stream %-4s identical (%d lines)" % (key, len(la)))
            continue
        same = False
        print("stream %-4s DIFFERS (%d / %d lines)" % (key, len(la), len(lb)))
        for d in list(difflib.unified_diff(la, lb, a, b, lineterm="", n=2))[:60]:
            print("    " + d)
    print("waits without an earlier record: %d / %d%s" % (len(ua), len(ub), "" if ua == ub else "  DIFFERENT"))
    for u in ua if ua == ub else sorted(set(ua) ^ set(ub)):
        print("    " + u)
    print("%d / %d trace lines: %s" % (na, nb, "IDENTICAL per stream" if same and ua == ub else "NOT identical"))
    return 0 if same and ua == ub else 1


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
