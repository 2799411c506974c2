"""The GEMM kernel families, one build of the library or several side by side: a sha256 of every arm's output per library and,
without --small, device-event times -- the same seeded inputs for each library, the libraries taking turns within every repetition.
usage: python tools/gemm_refactor_time.py [--small] [--reps N] [--only SUBSTR] [--out FILE] lib.so [lib.so ...]
With one library (or none: the shipped one) the hash lines are the bit-identity check of a new main loop / epilogue against another
run's (two settings of the library's knobs, two builds): diff the lines.
An arm is a set of LD_GEMM_* knobs (re-read per call: LD_TUNING=1) plus a call: the four DiT GEMMs with their real epilogues and
the fused qkv split, a ragged shape, one workgroup per tile, the half-tile route with every epilogue kind, an 8-phase convolution
with and without GroupNorm partials, the MXFP8 kernel with each of its epilogues; on the libraries whose file name contains
"variants" also the 512 x 128 tile and the software-pipelined loop.  --small: shapes of a few tiles per CU at most, the 8-phase
loop forced onto them (LD_GEMM_TILE=8), hashes only.
Give two copies of one build (two files: the loader hands out one handle per file) as the libraries after the first: per arm the table
then shows, per repetition and against the second library, the first library's difference (new - old) next to the third's
(old - old); "within" = the median of the first lies inside the [min .. max] of the old - old differences of the run."""
import hashlib, os, statistics, sys
os.environ["LD_TUNING"] = "1"
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from landiff_amd import _lib, ops

args = sys.argv[1:]
small = "--small" in args
opt = lambda name, default: args[args.index(name) + 1] if name in args else default
reps, only, out_path = int(opt("--reps", "10")), opt("--only", ""), opt("--out", "")
paths = [a for a in args if a.endswith(".so")] or [_lib.LIB_PATH]
libs = []
for path in paths:                       # one binding per file; ops.* calls whichever _lib._lib names
    _lib._lib, _lib.LIB_PATH = None, path
    libs.append(_lib.load())
dev, BF = torch.device("cuda:0"), torch.bfloat16
KNOBS = ("LD_GEMM_TILE", "LD_GEMM_PERSIST", "LD_GEMM_SP", "LD_GEMM_M512", "LD_GEMM_MSPLIT", "LD_GEMM_8P", "LD_GEMM_MX8P")
torch.manual_seed(0)
rnd = lambda *s, sc=1.0: (torch.randn(*s, device=dev) * sc).to(BF)

# DiT: CFG pair of 17776 tokens, D = 1920, 30 heads.  --small: 129 tile rows, so that N = 1024 still leaves two whole rounds + a tail
B, Ntok, D, H = (2, 16416, 1024, 16) if small else (2, 17776, 1920, 30)
M, Npad = B * Ntok, (Ntok + 127) // 128 * 128
x, x4, gate, resid, add2, mulv = rnd(M, D), rnd(M, 4 * D), rnd(B, 12 * D), rnd(M, D), rnd(M, D), rnd(M, D)
w_qkv, w_d, w_ff1, w_ff2 = rnd(3 * D, D, sc=0.02), rnd(D, D, sc=0.02), rnd(4 * D, D, sc=0.02), rnd(D, 4 * D, sc=0.02)
b_qkv, b_d, b_ff1 = rnd(3 * D), rnd(D), rnd(4 * D)
ln = tuple(rnd(64) for _ in range(4))
g1 = dict(resid=resid, gate=gate, gate_bstride=12 * D, gate_off_img=2 * D, gate_off_txt=8 * D, rows_per_batch=Ntok, text_len=226)
g2 = dict(g1, gate_off_img=5 * D, gate_off_txt=11 * D, add2=add2)
Mr, Nr, Kr = (16421, 1912, 1024) if small else (70003, 1000, 1024)      # ragged: M, N no multiples of the tile, N % 8 == 0
xr, wr_, br = rnd(Mr, Kr), rnd(Nr, Kr, sc=0.03), rnd(Nr)
# convolutions: 3 x 3 x 3, Cin = Cout = 256 on the 8-phase loop; Cin = Cout = 128 on the 512 x 128 tile (variants build), which
# takes no fewer than 256 tiles
conv_thw = {256: (2, 64, 64) if small else (4, 240, 360), 128: (2, 240, 360)}
conv_x = {c: torch.zeros(t + 2, h + 2, w + 2, c, device=dev, dtype=BF) for c, (t, h, w) in conv_thw.items()}
for c, thw in conv_thw.items(): conv_x[c][1:-1, 1:-1, 1:-1] = rnd(*thw, c)
conv_w = {c: rnd(c, 3, 3, 3, c, sc=0.02) for c in (256, 128)}
conv_b = {c: rnd(c) for c in (256, 128)}
_lib._lib = libs[0]                      # MXFP8 operands (the quantisers are not under test: made once, by the first library)
mx = {name: ops.quantize_mxfp8(t) for name, t in (("x", x), ("x4", x4), ("qkv", w_qkv), ("d", w_d), ("ff1", w_ff1), ("ff2", w_ff2))}


def qkv_heads(fn, *operands):
    q = torch.zeros(B, H, Npad, 64, device=dev, dtype=BF); k = torch.zeros_like(q); vt = torch.zeros(B, H, 64, Npad, device=dev, dtype=BF)
    fn(*operands, b_qkv, q, k, vt, B, Ntok, H, Npad, ln)
    return q, k, vt


def mx_out():
    o, s = torch.empty(M, 4 * D, device=dev, dtype=torch.uint8), torch.empty(4 * D // 128, M, 4, device=dev, dtype=torch.uint8)
    ops.gemm_mxfp8(*mx["x"], *mx["ff1"], out=o, out_scales=s, bias=b_ff1, act="gelu_tanh")
    return o, s


def conv(c, gn):
    r = ops.conv_cl(conv_x[c], conv_w[c], *conv_thw[c], gn_partials=gn, bias=conv_b[c])
    return r if gn else (r,)


# (name, knobs, call -> tuple of outputs, variants build only)
ARMS = [("qkv split", {}, lambda: qkv_heads(ops.gemm_qkv_heads, x, w_qkv), False),
        ("proj gate", {}, lambda: (ops.gemm(x, w_d, bias=b_d, **g1),), False),
        ("ff1 gelu", {}, lambda: (ops.gemm(x, w_ff1, bias=b_ff1, act="gelu_tanh"),), False),
        ("ff2 gate+add2", {}, lambda: (ops.gemm(x4, w_ff2, bias=b_d, **g2),), False),
        ("no epilogue", {}, lambda: (ops.gemm(x, w_d),), False),
        ("ragged gelu", {}, lambda: (ops.gemm(xr, wr_, bias=br, act="gelu_tanh"),), False),
        ("ff1 gelu PERSIST=0", {"LD_GEMM_PERSIST": "0"}, lambda: (ops.gemm(x, w_ff1, bias=b_ff1, act="gelu_tanh"),), False),
        ("half tiles bias", {"LD_GEMM_MSPLIT": "3"}, lambda: (ops.gemm(x, w_qkv, bias=b_qkv),), False),
        ("half tiles gelu", {"LD_GEMM_MSPLIT": "3"}, lambda: (ops.gemm(x, w_d, bias=b_d, act="gelu_tanh"),), False),
        ("half tiles gate", {"LD_GEMM_MSPLIT": "3"}, lambda: (ops.gemm(x4, w_ff2, bias=b_d, **g2),), False),
        ("half tiles generic", {"LD_GEMM_MSPLIT": "3"}, lambda: (ops.gemm(x, w_d, bias=b_d, act="gelu_tanh", mul=mulv),), False),
        ("half tiles qkv split", {"LD_GEMM_MSPLIT": "3"}, lambda: qkv_heads(ops.gemm_qkv_heads, x, w_qkv), False),
        ("conv 256", {}, lambda: conv(256, False), False), ("conv 256 + GN partials", {}, lambda: conv(256, True), False),
        ("mx bias", {}, lambda: (ops.gemm_mxfp8(*mx["x"], *mx["d"], bias=b_d),), False),
        ("mx gelu", {}, lambda: (ops.gemm_mxfp8(*mx["x"], *mx["ff1"], bias=b_ff1, act="gelu_tanh"),), False),
        ("mx gate+add2", {}, lambda: (ops.gemm_mxfp8(*mx["x4"], *mx["ff2"], bias=b_d, **g2),), False),
        ("mx generic", {}, lambda: (ops.gemm_mxfp8(*mx["x"], *mx["d"], bias=b_d, act="gelu_tanh", mul=mulv),), False),
        ("mx gelu -> mxfp8", {}, mx_out, False),
        ("mx qkv split", {}, lambda: qkv_heads(ops.gemm_qkv_heads_mxfp8, *mx["x"], *mx["qkv"]), False),
        ("m512 conv 128", {"LD_GEMM_M512": "1", "LD_GEMM_TILE": None}, lambda: conv(128, False), True),
        ("sp ff1 gelu", {"LD_GEMM_SP": "1"}, lambda: (ops.gemm(x, w_ff1, bias=b_ff1, act="gelu_tanh"),), True),
        ("sp proj gate", {"LD_GEMM_SP": "1"}, lambda: (ops.gemm(x, w_d, bias=b_d, **g1),), True),
        ("sp qkv split", {"LD_GEMM_SP": "1"}, lambda: qkv_heads(ops.gemm_qkv_heads, x, w_qkv), True)]


def run(lib, knobs, call):
    _lib._lib = lib
    for name in KNOBS: os.environ.pop(name, None)
    if small: os.environ["LD_GEMM_TILE"] = "8"
    for name, v in knobs.items():
        if v is None: os.environ.pop(name, None)
        else: os.environ[name] = v
    return call()


lines = []
def say(s=""):
    print(s, flush=True); lines.append(s)


say((f"small shapes M={M} D={D}" if small else f"DiT shapes M={M} D={D}") + "; libraries: " + ", ".join(f"[{i}] {p}" for i, p in enumerate(paths)))
differ = 0
for name, knobs, call, variants_only in ARMS:
    if only not in name: continue
    mine = [i for i, p in enumerate(paths) if not variants_only or "variants" in os.path.basename(p)]
    if not mine: continue
    hashes = []
    for i in mine:
        h = hashlib.sha256()
        for t in run(libs[i], knobs, call): h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
        hashes.append(h.hexdigest())
    same = len(set(hashes)) == 1
    differ += not same
    line = f"{name:22s} libs {mine} sha256 {hashes[0][:16]} " + ("all equal" if same else "DIFFER: " + " ".join(x[:16] for x in hashes))
    if not small:
        times = {i: [] for i in mine}
        for rep in range(reps + 2):                                 # the first two rounds warm up
            for i in mine[rep % len(mine):] + mine[:rep % len(mine)]:   # the starting library rotates
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(3): run(libs[i], knobs, call)
                e1.record(); torch.cuda.synchronize()
                if rep >= 2: times[i].append(e0.elapsed_time(e1) / 3 * 1e3)
        line += "\n    us, median [min .. max] of %d x 3: " % reps + "  ".join(
            f"[{i}] {statistics.median(v):7.1f} [{min(v):7.1f} .. {max(v):7.1f}]" for i, v in times.items())
        if len(mine) >= 3:
            a, b, c = mine[:3]
            d_new = [p - q for p, q in zip(times[a], times[b])]
            d_old = [p - q for p, q in zip(times[c], times[b])]
            ok = min(d_old) <= statistics.median(d_new) <= max(d_old)
            line += (f"\n    per repetition, [{a}] - [{b}]: median {statistics.median(d_new):+6.1f}   [{c}] - [{b}]: median {statistics.median(d_old):+6.1f} "
                     f"[{min(d_old):+6.1f} .. {max(d_old):+6.1f}]   " + ("within the old-vs-old spread" if ok else "OUTSIDE the old-vs-old spread"))
    say(line)
say("every arm: equal hashes across its libraries" if not differ else f"{differ} arm(s) DIFFER")
if out_path:
    with open(out_path, "w") as f: f.write("\n".join(lines) + "\n")
sys.exit(1 if differ else 0)
