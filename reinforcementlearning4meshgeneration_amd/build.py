"""Builds libmeshenv_hip.so (gfx950) in-tree with hipcc.  `python -m reinforcementlearning4meshgeneration_amd.build`."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG_DIR, "csrc")
LIB_NAME = "libmeshenv_hip.so"
LIB_PATH = os.path.join(PKG_DIR, LIB_NAME)
SOURCES = ["meshenv_hip.hip"]
ARCH = "gfx950"
PUBLIC_HEADERS = ["meshenv.h", "meshenv_optim.h", "meshenv_td3_actor_grad.h", "meshenv_ppo_grad.h", "meshenv_rollout.h",
                  "meshenv_onpolicy_train.h", "meshenv_offpolicy_train.h", "meshenv_offpolicy_learn.h",
                  "meshenv_eval_callback.h", "meshenv_onpolicy_learn.h", "meshenv_topology.h", "meshenv_fnn.h", "meshenv_fnn_train.h",
                  "meshenv_augment.h", "meshenv_ddpg.h", "meshenv_ddpg_grad.h"]     # include/: the C-ABI the translation unit implements

# -ffp-contract=off: the reference is CPython float arithmetic, which never fuses a*b+c.
# -fhip-fp32-correctly-rounded-divide-sqrt: numpy's float32 round() divides in IEEE float32.
# -mllvm -disable-machine-licm: the kernels' loops run once or twice (64-vertex chunks of a ring); hoisting constant
# materialisation out of them only lengthens live ranges (k_step<false>: 94 -> 89 VGPRs, 86 -> 78 spilled SGPRs;
# measured +1..3 % in the throughput workloads, neutral on the headline: profiles/r03_ab_all.log).
# -mllvm -amdgpu-atomic-optimizer-strategy=None: the LDS atomics of the observation scan (find_next_state) have one to
# three active lanes; the optimiser's wave reduction in front of them is the very DPP sequence they replace
# (headline 14.58 -> 14.42 us, 65 536 envs +1 %, rollout +2 %; tools/ab_all.sh).
# -mllvm -amdgpu-kernarg-preload-count=16: leading plain kernel arguments (up to 14 dwords on gfx950) are in scalar registers
# when a wave starts.  The CU-group step kernels take what their entry needs that way (EntryArgs, csrc/meshenv_kernels.h) and
# request an environment's ring and record without a scalar round trip in front; the flag holds for the whole translation
# unit, so every other kernel with leading pointer or integer arguments is preloaded as well.
HIPCC_FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
               "-fno-fast-math", "-fPIC", "-shared", f"--offload-arch={ARCH}", "-Wall", "-Wno-unused-function",
               "-mllvm", "-disable-machine-licm", "-mllvm", "-amdgpu-atomic-optimizer-strategy=None",
               "-mllvm", "-amdgpu-kernarg-preload-count=16"]


def hipcc_path() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (need ROCm to build libmeshenv_hip.so)")


def needs_build() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    # every header of csrc/ is a dependency of the one translation unit (meshenv_hip.hip includes them all)
    deps = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip"))]
    deps += [os.path.join(os.path.dirname(PKG_DIR), "include", h) for h in PUBLIC_HEADERS]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False, extra_flags=()) -> str:
    if not force and not needs_build():
        return LIB_PATH
    cmd = [hipcc_path(), *HIPCC_FLAGS, *extra_flags, "-o", LIB_PATH] + [os.path.join(CSRC, s) for s in SOURCES]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd, cwd=CSRC)
    # what this binary was built from (tools/source_state.py: a profile refuses to describe a library that is not the sources')
    import hashlib
    import json
    h = hashlib.sha256()
    root = os.path.dirname(PKG_DIR)
    files = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".hip"))) + [os.path.join(root, "include", h) for h in PUBLIC_HEADERS]
    for f in files:
        h.update(os.path.relpath(f, root).encode())
        h.update(open(f, "rb").read())
    json.dump({"source_sha256": h.hexdigest(), "flags": [*HIPCC_FLAGS, *extra_flags]}, open(LIB_PATH + ".source", "w"))
    return LIB_PATH


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
