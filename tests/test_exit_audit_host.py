"""CPU (needs hipcc, no GPU): register budget of the kernels whose epilogues carry the row-group reduce-scatter.  The lean GEMV
unit and the attention unit are compiled for gfx950 with the library's own flags and -Rpass-analysis=kernel-resource-usage, and
the compiler's per-kernel report is read:

  * no scratch and no VGPR spill in any gemv_fast_kernel instantiation with KR <= 8, nor in any attention kernel;
  * the twelve MODE 1, KR = 16 instantiations (the whole 16384-wide vector cached in registers) spilled before the exit audit
    already — 276 to 344 bytes per lane, the figures of PARENT_SCRATCH below — and may not spill more than they did.
"""
import concurrent.futures
import re
import subprocess

from teal_amd import _lib

# scratch bytes per lane of the MODE 1, KR = 16 instantiations before the exit audit, by (PAIR, EXACT, ROPE); the same for both
# tile widths (LPR 8 and 16)
PARENT_SCRATCH = {(False, False, False): 276, (False, False, True): 280, (False, True, False): 332, (False, True, True): 344,
                  (True, False, False): 276, (True, True, False): 332}


def _resource_usage(unit):
    """{mangled kernel name: {"scratch": bytes per lane, "vgpr_spill": n, "sgpr_spill": n}} of one translation unit"""
    base = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-pass-failed", f"-I{_lib.INCLUDE}", f"-I{_lib.CSRC}",
            *_lib.NO_PACKED_FP32, _lib.FP_CONTRACT]
    if unit in _lib.PRELOAD:
        base += ["-mllvm", f"-amdgpu-kernarg-preload-count={_lib.PRELOAD[unit]}"]
    r = subprocess.run([_lib._hipcc(), *base, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                        f"{_lib.CSRC}/{unit}", "-o", "/dev/null"], stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill): (\d+)", ln)
        if m and cur is not None:
            cur[{"ScratchSize [bytes/lane]": "scratch", "VGPRs Spill": "vgpr_spill", "SGPRs Spill": "sgpr_spill"}[m.group(1)]] = int(m.group(2))
    return out


def test_epilogue_kernels_keep_their_register_budget():
    with concurrent.futures.ThreadPoolExecutor(max_workers=2) as ex:
        fast, att = ex.map(_resource_usage, ("teal_gemv_fast_f16.hip", "teal_attention.hip"))
    lean = {k: v for k, v in fast.items() if "gemv_fast_kernel" in k}
    assert len(lean) >= 40 and all(set(v) == {"scratch", "vgpr_spill", "sgpr_spill"} for v in list(lean.values()) + list(att.values()))
    spilling = 0
    for name, use in sorted(lean.items()):
        # template <bool BF16, int MODE, bool PAIR, int LPR, int KR, bool EXACT, bool PHASE, int U, bool W8, bool ROPE>
        args = [int(v) for v in re.findall(r"L[bi](\d+)E", name.split("gemv_fast_kernelI")[1].split("EEv")[0] + "E")]
        assert len(args) == 10, name
        _, mode, pair, lpr, kr, exact, _, _, _, rope = args
        print(f"RESOURCE gemv_fast_kernel MODE={mode} PAIR={pair} LPR={lpr} KR={kr} EXACT={exact} ROPE={rope}: scratch {use['scratch']} "
              f"B/lane, VGPR spill {use['vgpr_spill']}")
        if kr <= 8:
            assert use["scratch"] == 0 and use["vgpr_spill"] == 0, (name, use)
        else:
            assert mode == 1 and kr == 16, name
            spilling += 1
            assert use["scratch"] <= PARENT_SCRATCH[(bool(pair), bool(exact), bool(rope))], (name, use)
    assert spilling == 12
    kernels = [k for k in att if "attention" in k]
    assert len(kernels) >= 20
    for name in kernels:
        print(f"RESOURCE {name[:60]}: scratch {att[name]['scratch']} B/lane, VGPR spill {att[name]['vgpr_spill']}")
        assert att[name]["scratch"] == 0 and att[name]["vgpr_spill"] == 0, (name, att[name])
