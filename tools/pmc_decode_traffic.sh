#!/bin/bash
# HBM traffic of EVERY kernel of the decode step from PMC counters, inside a real bench.py run (round 3).
# Collected as MI355X_MICROARCH.md (section HBM) prescribes: separate rocprofv3 --pmc passes (nothing but --kernel-trace beside
# them), FETCH_SIZE doubled on gfx950 (128-B requests are tallied at 64 B), WRITE_SIZE as is, TCC_EA0_RDREQ_sum x 128 B as the
# cross-check.  The program itself follows `--` (no wrapper hop).  Writes gpurun_out/r06p/r06_pmc_decode_traffic.json.
set -u
ROOT=${GRAFT_REPO_ROOT:-/root/repo}
COMMIT=${1:-unknown}
mkdir -p $ROOT/gpurun_out/r06p
cd /tmp && export TMPDIR=/tmp
for C in FETCH_SIZE WRITE_SIZE TCC_EA0_RDREQ_sum; do
  rm -rf /tmp/pmcd_$C
  timeout 900 rocprofv3 --kernel-trace --pmc $C -d /tmp/pmcd_$C -o p -- python3 $ROOT/bench.py --full --steps 1 --warmup 0 --new 12 --no-cpu-baseline --no-graph > /tmp/pmcd_$C.log 2>&1
  rc=$?; if [ $rc -ne 0 ]; then echo "pass $C failed ($rc): no further GPU passes"; exit $rc; fi
done
python3 - "$COMMIT" "$ROOT" <<'PY'
import glob, json, os, re, sqlite3, sys
# LLaMA-2-7B, ctx ~2175.  Bytes per launch of a matrix: 2 per weight, or the w13 image's (csrc/p13.h: RT + LO + NIB + SGN, each section
# rounded up to 256 bytes; the few escaped rows of ESC are left out) when the kernel that ran is a p13_t instantiation.
SHAPES = {"gateup_gemv": (2 * 11008, 4096), "qkv_rope_gemv": (12288, 4096), "o_gemv": (4096, 4096), "down_gemv": (4096, 11008), "lm_head_gemv": (32000, 4096)}
def up(v): return (v + 255) // 256 * 256
def matrix_bytes(key, name):
    N, K = SHAPES[key]
    return (up(4 * N) + up(N * K) + up(N * K // 2) + up(N * K // 8)) if "p13_t" in name else 2 * N * K
def targs(n):           # template arguments of the kernel name
    m = re.search(r"<(.*?)>\(", n) or re.search(r"<(.*)>", n)
    return [a.strip() for a in m.group(1).split(",")] if m else []
# gemv_kernel<T, TO, WT, R, U, PF, NT, SWIGLU, XPT>: gate/up is the SwiGLU form (whatever PF is: the image kernel runs without the prefetch),
# lm_head the fp32-output form.  Where several instantiations match (bench.py --full also runs a decode_pack-off phase), the one with
# the most launches is the one the default path runs.
MATCH = {
    "gateup_gemv": lambda n: "gemv_kernel<" in n and len(targs(n)) == 9 and targs(n)[7] == "true",
    "qkv_rope_gemv": lambda n: "gemv_qkv_rope_kernel<" in n,
    "lm_head_gemv": lambda n: "gemv_kernel<" in n and len(targs(n)) == 9 and targs(n)[1] == "float",
    "attn_decode_partial": lambda n: "attn_decode_partial_kernel<" in n,
    "attn_decode_combine": lambda n: "attn_decode_combine_kernel<" in n,
}
ATTN_BYTES = 2 * 32 * 2175 * 128 * 2
COUNTERS = ("FETCH_SIZE", "WRITE_SIZE", "TCC_EA0_RDREQ_sum")
vals = {}               # counter -> kernel name -> values of every launch
for c in COUNTERS:
    vals[c] = {}
    dbs = glob.glob(f"/tmp/pmcd_{c}/**/*.db", recursive=True)
    if dbs:
        for name, v in sqlite3.connect(dbs[0]).cursor().execute("select kernel_name, value from counters_collection where counter_name = ?", (c,)):
            vals[c].setdefault(name, []).append(v)
def mean(v): return sum(v) / len(v) if v else 0.0
def entry(key, name, pick=lambda c, v: v):
    """one kernel's summary from the launches of `name`; pick(counter, values) selects the launches that belong to `key`"""
    f, w, r = (pick(c, vals[c].get(name, [])) for c in COUNTERS)
    alg = matrix_bytes(key, name) if key in SHAPES else (ATTN_BYTES if key == "attn_decode_partial" else None)
    e = {"algorithmic_bytes": alg, "kernel": name[:140], "launches_sampled": len(f), "FETCH_SIZE_KB_avg": mean(f), "WRITE_SIZE_KB_avg": mean(w),
         "TCC_EA0_RDREQ_sum_avg": mean(r), "hbm_bytes_per_launch": int(2 * mean(f) * 1024 + mean(w) * 1024), "rdreq_bytes_per_launch": int(mean(r) * 128)}
    if key in SHAPES:
        e["bytes_16bit"] = 2 * SHAPES[key][0] * SHAPES[key][1]
    if alg:
        e["traffic_over_algorithmic"] = round(e["hbm_bytes_per_launch"] / alg, 4)
    return e
def most_launched(match):
    names = [n for n in vals["FETCH_SIZE"] if match(n)]
    return max(names, key=lambda n: len(vals["FETCH_SIZE"][n]))
out = {"source": "tools/pmc_decode_traffic.sh: three separate rocprofv3 --kernel-trace --pmc passes over `python3 bench.py --full --steps 1 --warmup 0 --new 12 --no-cpu-baseline --no-graph` (rounds 3-4)",
       "commit": sys.argv[1], "csrc_sha16": __import__("subprocess").check_output(["python3", os.path.join(sys.argv[2], "tools", "src_hash.py")]).decode().strip(),
       "correction": "gfx950: read bytes = 2 * FETCH_SIZE * 1024 (128-B requests tallied at 64 B) + WRITE_SIZE * 1024; cross-check TCC_EA0_RDREQ_sum * 128 B",
       "algorithmic_bytes": "what the kernel that ran streams: 2 bytes per weight, or the w13 image (0.8125 x + the row table) for a p13_t instantiation; bytes_16bit is the former",
       "kernels": {}}
for key, match in MATCH.items():
    try:
        out["kernels"][key] = entry(key, most_launched(match))
    except Exception as ex:  # noqa: BLE001
        out["kernels"][key] = {"error": str(ex)}
# split-K: gemv_splitk_kernel<T, TO, WT, R, U, NT>.  On the 16-bit matrices o and down are two instantiations (U = 2 and U = 6); on the images
# both run U = 2 -- one kernel name, launched o, down, o, down, ... -- and differ by what they read: down streams 2.7 x o's bytes, so
# the launches of a read counter fall into two groups around the midpoint of its range (asserted: each group within 20 % of its mean).
# Both write the same 4096 outputs: WRITE_SIZE is taken over all launches.
try:
    sk = most_launched(lambda n: "gemv_splitk_kernel<" in n)
    fv = vals["FETCH_SIZE"][sk]
    if max(fv) > 1.5 * min(fv):                                   # one instantiation for both matrices
        def side(high):
            def pick(c, v):
                if c == "WRITE_SIZE" or not v:
                    return v
                mid = (min(v) + max(v)) / 2
                g = [x for x in v if (x > mid) == high]
                assert g and all(abs(x - mean(g)) <= 0.2 * mean(g) for x in g), f"{c}: the launches of {sk[:60]} do not fall into two groups"
                return g
            return pick
        out["kernels"]["o_gemv"] = entry("o_gemv", sk, side(False))
        out["kernels"]["down_gemv"] = entry("down_gemv", sk, side(True))
        n_o, n_d = out["kernels"]["o_gemv"]["launches_sampled"], out["kernels"]["down_gemv"]["launches_sampled"]
        assert n_o == n_d, f"o and down launches differ: {n_o} / {n_d}"
    else:
        for key, u in (("o_gemv", "2"), ("down_gemv", "6")):
            out["kernels"][key] = entry(key, most_launched(lambda n, u=u: "gemv_splitk_kernel<" in n and targs(n)[3:5] == ["2", u]))
except Exception as ex:  # noqa: BLE001
    out["kernels"]["o_gemv"] = out["kernels"]["down_gemv"] = {"error": str(ex)}
bad = [k for k, e in out["kernels"].items() if "error" in e]
gu = out["kernels"].get("gateup_gemv", {})
out["hbm_bytes_per_launch"] = gu.get("hbm_bytes_per_launch")        # the dominant kernel: bench.py's roofline.traffic
out["kernel"] = gu.get("kernel", "?").split("(")[0] + " N=22016 K=4096 (decode rmsnorm + gate/up + SwiGLU)"
json.dump(out, open(os.environ.get("GRAFT_REPO_ROOT", "/root/repo") + "/gpurun_out/r06p/r06_pmc_decode_traffic.json", "w"), indent=1)
print(json.dumps(out)[:3000])
if bad:
    sys.exit(f"no figure for {bad}: do not commit this summary")
PY
