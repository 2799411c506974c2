"""The pipelined attention kernels, one build of the library or several side by side: a sha256 of every arm's output and, at the DiT
launch, device-event times -- the same seeded inputs for each library, the libraries taking turns within every repetition.
usage: python tools/attn_refactor_time.py [--small] [--reps N] [--only SUBSTR] [--out FILE] lib.so [lib.so ...]
An arm is a set of LD_ATTN_* knobs (re-read per call: LD_TUNING=1) plus the entry point.  Arms of the variants build (128-row
tile, round-1 pipeline) run on the libraries whose file name contains "variants", every other arm on all of them.
Give two copies of one build (two files: the loader hands out one handle per file) as the libraries after the first: per arm the table
then shows, per repetition and against the second library, the first library's difference (new - old) next to the third's
(old - old); "within" = the median of the first does not exceed the largest old - old difference of the run."""
import hashlib, os, statistics, sys
os.environ["LD_TUNING"] = "1"
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from landiff_amd import _lib, ops

args = sys.argv[1:]
small = "--small" in args
opt = lambda name, default: args[args.index(name) + 1] if name in args else default
reps, only, out_path = int(opt("--reps", "20")), opt("--only", ""), opt("--out", "")
paths = [a for a in args if a.endswith(".so")] or [_lib.LIB_PATH]
libs = []
for path in paths:                       # one binding per file; ops.* calls whichever _lib._lib names
    _lib._lib, _lib.LIB_PATH = None, path
    libs.append(_lib.load())
dev, BF = torch.device("cuda:0"), torch.bfloat16
KNOBS = ("LD_ATTN_VARIANT", "LD_ATTN_Q64", "LD_ATTN_Q128", "LD_ATTN_SAFE", "LD_ATTN_DYN", "LD_ATTN_MSUM", "LD_ATTN_NW", "LD_ATTN_NPRE")

# (name, knobs, entry, variants build only, timing gates the shipped arms)
ARMS = [("q64 dynamic", {}, "dense", False, True), ("q64 static", {"LD_ATTN_DYN": "0"}, "dense", False, True),
        ("window dynamic", {}, "window", False, True), ("window static", {"LD_ATTN_DYN": "0"}, "window", False, False),
        ("exact", {}, "exact", False, True), ("forced safe pass", {"LD_ATTN_SAFE": "1"}, "dense", False, False),
        ("p16 w4", {"LD_ATTN_Q64": "0"}, "dense", False, True), ("p16 w8", {"LD_ATTN_Q64": "0", "LD_ATTN_NW": "8"}, "dense", False, False),
        ("p16 MSUM=0", {"LD_ATTN_Q64": "0", "LD_ATTN_MSUM": "0"}, "dense", False, False)]
ARMS += [(f"q128 npre {n}", {"LD_ATTN_Q128": "2", "LD_ATTN_NPRE": str(n)}, "dense", True, False) for n in (44, 36, 52, 1036, 1040)]
ARMS += [("pipe2 w4", {"LD_ATTN_VARIANT": "8"}, "dense", True, False), ("pipe2 w8", {"LD_ATTN_VARIANT": "8", "LD_ATTN_NW": "8"}, "dense", True, False)]

# DiT launch: CFG pair, 30 heads, text 226 + 13 frames of 1350 tokens, window of 2 frames (tools/attn_window_time.py).  --small: the
# shapes of the tests (ragged / exact / empty last half tile / 6 tiles; N = 1122 and 1890 are 4 m + 2 tiles, which pipe2 needs) and
# one with enough heads for the dynamic form (>= 4 rounds of the chip's slots).  (B, H, N, window prefix, group, frames)
SHAPES = [(1, 3, 1122, 90, 100, 1), (2, 1, 1408, 64, 200, 1), (1, 2, 2065, 128, 320, 1), (1, 1, 384, 0, 64, 6), (2, 128, 1890, 90, 200, 1)] if small \
    else [(2, 30, 17776, 226, 1350, 2)]


def make(B, H, N):
    g = torch.Generator().manual_seed(1000 + N)
    Npad = (N + 127) // 128 * 128
    q, k = torch.zeros(B, H, Npad, 64, dtype=BF), torch.zeros(B, H, Npad, 64, dtype=BF)
    vt = torch.zeros(B, H, 64, Npad, dtype=BF)
    q[:, :, :N] = torch.randn(B, H, N, 64, generator=g).to(BF); k[:, :, :N] = torch.randn(B, H, N, 64, generator=g).to(BF)
    vt[:, :, :, :N] = torch.randn(B, H, 64, N, generator=g).to(BF)
    return q.to(dev), k.to(dev), vt.to(dev), torch.zeros(B, N, H * 64, device=dev, dtype=BF)


def run(lib, knobs, entry, t, shape):
    _lib._lib = lib
    for name in KNOBS: os.environ.pop(name, None)
    os.environ.update(knobs)
    B, H, N, P, G, w = shape
    q, k, vt, out = t
    if entry == "window": ops.attn_fwd_window(q, k, vt, out, N, 0.125, P, G, w)
    else: ops.attn_fwd(q, k, vt, out, N, N, 0.125, exact=entry == "exact")
    return out


lines = []
def say(s=""):
    print(s, flush=True); lines.append(s)


say(("small shapes" if small else f"DiT launch B={SHAPES[0][0]} H={SHAPES[0][1]} N={SHAPES[0][2]}") + "; libraries: " + ", ".join(f"[{i}] {p}" for i, p in enumerate(paths)))
tensors = [make(*s[:3]) for s in SHAPES]
differ = 0
for name, knobs, entry, variants_only, gated in ARMS:
    if only not in name: continue
    mine = [i for i, p in enumerate(paths) if not variants_only or "variants" in os.path.basename(p)]
    if not mine: continue
    hashes, kernels = [], set()
    for i in mine:
        h = hashlib.sha256()
        for s, t in zip(SHAPES, tensors):
            if knobs.get("LD_ATTN_VARIANT") == "8" and ((s[2] + 63) // 64 - 2) % 4: continue      # pipe2 takes 4 m + 2 tiles only
            t[3].zero_()
            h.update(run(libs[i], knobs, entry, t, s).cpu().view(torch.int16).numpy().tobytes())
            kernels.add((libs[i].ld_attn_last_kernel() or b"").decode())
        hashes.append(h.hexdigest())
    same = len(set(hashes)) == 1
    differ += not same
    line = f"{name:18s} libs {mine} sha256 {hashes[0][:16]} " + ("all equal" if same else "DIFFER: " + " ".join(x[:16] for x in hashes)) + "  " + " ".join(sorted(kernels))
    if not small:
        s, t = SHAPES[0], tensors[0]
        times = {i: [] for i in mine}
        for rep in range(reps + 2):                                 # the first two rounds warm up
            for i in mine[rep % len(mine):] + mine[:rep % len(mine)]:   # the starting library rotates
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(3): run(libs[i], knobs, entry, t, s)
                e1.record(); torch.cuda.synchronize()
                if rep >= 2: times[i].append(e0.elapsed_time(e1) / 3 * 1e3)
        line += "\n    us, median [min .. max] of %d x 3: " % reps + "  ".join(
            f"[{i}] {statistics.median(v):7.1f} [{min(v):7.1f} .. {max(v):7.1f}]" for i, v in times.items())
        if len(mine) >= 3:
            a, b, c = mine[:3]
            d_new = [x - y for x, y in zip(times[a], times[b])]
            d_old = [x - y for x, y in zip(times[c], times[b])]
            ok = statistics.median(d_new) <= max(d_old)
            line += (f"\n    per repetition, [{a}] - [{b}]: median {statistics.median(d_new):+6.1f}   [{c}] - [{b}]: median {statistics.median(d_old):+6.1f} "
                     f"[{min(d_old):+6.1f} .. {max(d_old):+6.1f}]   " + ("within the old-vs-old spread" if ok else "OUTSIDE the old-vs-old spread")
                     + ("" if gated else "  (reported, not gated)"))
    say(line)
say("every arm: equal hashes across its libraries" if not differ else f"{differ} arm(s) DIFFER")
if out_path:
    with open(out_path, "w") as f: f.write("\n".join(lines) + "\n")
sys.exit(1 if differ else 0)
