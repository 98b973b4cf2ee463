"""Shared by tests/test_shim_lookahead_on_cpu.py and tests/test_gpu_shim_lookahead.py: builds tests/cpp/shim_lookahead_check.cpp (scripted
callers of erasor::OfflineMapUpdater's look-ahead) against a liberasor_hip.so -- the real one, or the recording stand-in
tests/cpp/fake_erasor_hip.cpp --, runs it, reads back what it wrote and checks what every script must satisfy.  Every comparison is
bitwise or an integer count."""
import os
import re
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SHIM = os.path.join(ROOT, "erasor_amd", "csrc", "shim")
DRIVER_SRC = os.path.join(HERE, "cpp", "shim_lookahead_check.cpp")
FAKE_SRC = os.path.join(HERE, "cpp", "fake_erasor_hip.cpp")
FIXED_POLICIES = ("window", "greedy", "greedy_deferred", "ticketless", "stop_and_go")
KEEPS_LOOKAHEAD = ("window", "greedy", "greedy_deferred")  # the policies that announce every node in time and hand every ticket in
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def n_nodes(interval, lookahead):
    return 3 * interval + lookahead + 3


def build_fake_lib(d):
    """the stand-in as <d>/liberasor_hip.so"""
    lib = os.path.join(d, "liberasor_hip.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", lib, FAKE_SRC])
    return lib


def build_driver(exe, libdir=None, sanitize=False):
    """the driver with erasor_shim.cpp and erasor_io.cpp, like tests/cpp/ros1_adapter_check without the ROS / PCL defines; linked against
    <libdir>/liberasor_hip.so, or (libdir None) with the stand-in compiled in"""
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-I" + SHIM] + (SANITIZE if sanitize else []) + ["-o", exe, DRIVER_SRC,
           os.path.join(SHIM, "erasor_shim.cpp"), os.path.join(SHIM, "erasor_io.cpp")]
    cmd += [FAKE_SRC] if libdir is None else ["-L" + libdir, "-lerasor_hip", "-Wl,-rpath," + libdir]
    subprocess.check_call(cmd)
    return exe


def write_pcd_binary(path, c):
    with open(path, "wb") as f:
        f.write(("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n"
                 "WIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA binary\n" % (len(c), len(c))).encode())
        f.write(np.ascontiguousarray(c, np.float32).tobytes())


def write_data(d, m, scans, poses):
    """map.pcd, scan%d.bin, poses.txt: the files tests/test_gpu_shim.py writes for the ROS1 adapter's check"""
    write_pcd_binary(os.path.join(d, "map.pcd"), m)
    with open(os.path.join(d, "poses.txt"), "w") as f:
        for k, (s, p) in enumerate(zip(scans, poses)):
            np.ascontiguousarray(s, np.float32).tofile(os.path.join(d, "scan%d.bin" % k))
            f.write(" ".join("%.17g" % v for v in p) + "\n")


def toy_data(d, n_scans=40, pts=12):
    """a sequence for the stand-in: every scan and every pose differs from every other"""
    rng = np.random.default_rng(7)
    m = rng.uniform(-5, 5, (16, 4)).astype(np.float32)
    scans = [(rng.uniform(-5, 5, (pts, 4)) + 100 * (k + 1)).astype(np.float32) for k in range(n_scans)]
    poses = []
    for k in range(n_scans):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        poses.append([0.5 * k, -0.25 * k, 0.01 * k] + list(q))
    write_data(d, m, scans, poses)
    return m, scans


class Script:
    pass


def run_driver(exe, data_dir, out_prefix, n_scans, interval, lookaheads, policy, seed0=0, n_seeds=1, timeout=120, env=None):
    """one process: a script per (seed, lookahead); returns the parsed scripts"""
    out = subprocess.run([exe, data_dir, out_prefix, str(n_scans), str(interval), ",".join(str(l) for l in lookaheads), policy, "%d:%d" % (seed0, n_seeds)],
                         capture_output=True, text=True, timeout=timeout, env=env)
    assert out.returncode == 0, "%s interval %d: exit %d\n%s" % (policy, interval, out.returncode, (out.stdout + out.stderr)[-4000:])
    scripts = parse(out_prefix)
    assert len(scripts) == n_seeds * len(lookaheads)
    for s in scripts:
        s.policy, s.interval, s.stderr = policy, interval, out.stderr
    return scripts, out


def parse(out_prefix):
    scripts = []
    raw = open(out_prefix + "res.bin", "rb").read()
    off = 0
    while off < len(raw):
        kind, a, b, nbytes = np.frombuffer(raw, np.int32, 4, off)
        off += 16
        payload = raw[off:off + nbytes]
        off += nbytes
        if kind == 1:
            s = Script()
            s.lookahead, s.seed, s.callbacks, s.final_map, s.threw, s.mismatches = int(a), int(b), [], None, None, None
            scripts.append(s)
        elif kind == 8:
            s.T = np.frombuffer(payload, np.uint32).reshape(int(a), 32)
        elif kind == 2:
            s.callbacks.append({"node": int(a)})
        elif kind in (3, 4):
            s.callbacks[-1]["map_rejected" if kind == 3 else "query_rejected"] = np.frombuffer(payload, np.uint32).reshape(-1, 4)
        elif kind == 5:
            s.callbacks[-1]["last"] = np.frombuffer(payload, np.uint64, 12)  # the counts of the result block (n_map_in .. n_dynamic)
            s.callbacks[-1]["last_bytes"] = bytes(payload)
        elif kind == 6:
            s.final_map = np.frombuffer(payload, np.uint32).reshape(-1, 4)
        elif kind == 7:
            s.threw, s.mismatches = int(a), int(b)
    k = -1
    for line in open(out_prefix + "log.txt").read().splitlines():
        if line.startswith("script "):
            k += 1
            scripts[k].log = []
            scripts[k].n_nodes = int(re.search(r"nodes=(\d+)", line).group(1))
        scripts[k].log.append(line)
    assert k + 1 == len(scripts)
    return scripts


def _fields(line):
    return dict(f.split("=") for f in line.split()[1:])


def tag(s):
    return "%s interval %d lookahead %d seed %d" % (s.policy, s.interval, s.lookahead, s.seed)


def failures(s):
    """what script s violates of (a) nothing throws, (c) / (d) look-ahead kept, (e) bookkeeping, and of (b) the processed nodes being
    exactly the ungated ones in order -- as a list of strings (empty: all hold).  WHAT each processed node computed is checked by
    check_against_stand_in / by the GPU test against the oracle."""
    bad = []
    N, iv = s.n_nodes, s.interval
    ungated = [k for k in range(N) if (k + 1) % iv == 0]
    if s.threw or any("threw=1" in l for l in s.log):
        bad.append("(a) threw: " + "; ".join(l for l in s.log if "threw=1" in l and not l.startswith("end")))
        return bad  # (the script ended there: the rest would only repeat it)
    if [c["node"] for c in s.callbacks] != ungated:
        bad.append("(b) processed %s, not %s" % ([c["node"] for c in s.callbacks], ungated))
    ticketed, by_ticket, calls = set(), {}, []
    for line in s.log[1:]:
        op, f = line.split()[0], _fields(line)
        if op == "end":
            end = f
            continue
        calls.append((op, f))
        if f["out"] != f["lib"]:
            bad.append("(e) after `%s`: outstanding() %s, the library holds %s" % (line, f["out"], f["lib"]))
        if op in ("announce_upcoming", "announce_next", "deferred_result") and f["ticket"] == "1":
            ticketed.add(int(f["node"]))
        if op == "callback_node":
            by_ticket[int(f["node"])] = int(f["byticket"])
            if int(f["processed"]) != (int(f["node"]) in ungated):
                bad.append("(b) callback %s processed=%s" % (f["node"], f["processed"]))
    if s.mismatches:
        bad.append("(e) %d calls left outstanding() different from the library's count" % s.mismatches)
    if sorted(by_ticket) != list(range(N)):
        bad.append("(b) callbacks %s" % sorted(by_ticket))
    if s.policy in KEEPS_LOOKAHEAD:
        gated_ticketed = sorted(k for k in ticketed if k not in ungated)
        if gated_ticketed:
            bad.append("(c) gated nodes %s were given a ticket" % gated_ticketed)
        lost = [k for k in ungated if k in ticketed and by_ticket.get(k) != 1]
        if lost:
            bad.append("(c) nodes %s held a ticket and were not stepped by it" % lost)
        if int(end["dropped"]) != 0:
            bad.append("(c) the updater dropped %s announcements" % end["dropped"])
        if int(end["stepped_by_ticket"]) != sum(by_ticket.get(k, 0) for k in ungated):
            bad.append("(c) stepped_by_ticket() %s" % end["stepped_by_ticket"])
        late = [k for k in ungated[1:] if by_ticket.get(k) != 1]
        if late:
            bad.append("(d) nodes %s, behind the first processed one, were not stepped by ticket" % late)
    return bad


def stand_in_failures(s, m, scans):
    """(b) on the stand-in: every processed node ran on its own cloud with its own two transforms, and the map says so too"""
    bad = []
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)  # noqa: E731
    for c in s.callbacks:
        k = c["node"] % len(scans)
        if not np.array_equal(c["map_rejected"], bits(scans[k][:8])):
            bad.append("(b) node %d ran on another cloud" % c["node"])
        if not np.array_equal(c["query_rejected"].reshape(-1), s.T[k]):
            bad.append("(b) node %d ran with other transforms" % c["node"])
    if not s.threw:
        want = np.concatenate([bits(m)] + [bits(scans[c["node"] % len(scans)][:1]) for c in s.callbacks])
        if s.final_map is None or not np.array_equal(s.final_map, want):
            bad.append("(b) final map")
    return bad
