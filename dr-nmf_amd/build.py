"""Build libdrnmf.so (hipcc, gfx950 only) in-tree next to this file.

    python dr-nmf_amd/build.py [--force]

hipcc cross-compiles without a GPU.  The .so is git-ignored but travels to the GPU box with the
repo snapshot.
"""
import fcntl
import glob
import hashlib
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libdrnmf.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# gfx950 only.  xnack-: what MI355X runs by default (XNACK off); the compiler then need not keep the
# address registers of in-flight loads intact for a replay: +0.6 % on the recurrent cell, +1.4 % on
# the GEMMs against the generic target.  A process with XNACK enabled (HSA_XNACK=1) cannot load it:
# set DRNMF_OFFLOAD_ARCH=gfx950 and rebuild.
ARCH = ["--offload-arch=" + os.environ.get("DRNMF_OFFLOAD_ARCH", "gfx950:xnack-")]
# DRNMF_TIMELINE=1: measurement build with s_memtime stamps in the cell kernels (tools/timeline.py)
# DRNMF_MEASURE=1: measurement build -- the ablation arguments / environment aids of DESIGN.md section 8 compiled in
FLAGS = ARCH + (["-DDRNMF_TIMELINE"] if os.environ.get("DRNMF_TIMELINE") else []) + \
    (["-DDRNMF_MEASURE"] if os.environ.get("DRNMF_MEASURE") else []) + os.environ.get("DRNMF_EXTRA_FLAGS", "").split() + ["-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function",
         # scalar kernel arguments arrive preloaded in SGPRs (no kernarg load on the critical path)
         "-mllvm", "-amdgpu-kernarg-preload-count=16",
         # `#pragma unroll` means it: with the default threshold the optimiser refused to unroll the output-tile
         # loops of gemm_nt_kernel under the powf epilogues of the general beta-divergence (24 "loop not
         # unrolled" warnings); acc[a][b] was then indexed dynamically = 832 bytes of scratch per lane
         "-mllvm", "-pragma-unroll-threshold=262144"]


# Kernels that must not spill: source -> kernel name, or a tuple of names (each must be seen).  These sources are compiled with
# -Rpass-analysis=kernel-resource-usage and the build fails if a matching kernel reports scratch.
NO_SCRATCH = {# (lstm_cot_rows_kernel: the head's backward for a given mask cotangent, include/drnmf_waveloss.h)
              "lstm.hip": ("lstm_step_kernel", "lstm_cot_rows_kernel"),
              # the tile kernel keeps H, num and den of its tiles in registers; the pack / zero kernels ride along
              "snmf_mask.hip": "snmf_mask_",
              # its fp16-operand sibling: H (fp32 master), num and den of its tiles in registers as well
              "snmf_f16.hip": "snmf_f16_",
              # the adaptive baseline's H pass keeps num and den in registers, its statistics pass four accumulators per
              # 16-atom tile; the small kernels of the file ride along
              "snmf_adapt.hip": "snmf_adapt_",
              # the online form: the fixed tile kernel's registers in its H kernel, two accumulators per 16-atom tile
              # in its statistics kernel
              "snmf_online.hip": "snmf_online_",
              # the KL tile kernel: H's numerator of its tiles, the column denominators and a chunk of V in registers
              "snmf_kl.hip": "snmf_kl_",
              # the target kernels keep the noisy member's bins of a frame in registers (up to 27 per lane)
              # (the transposed inverse runs the frame bodies with a register-only epilogue)
              "stft.hip": ("stft_pair_target_", "istft_vjp_"),
              # the mask head's backward for a given cotangent
              "train.hip": "cot_grad_kernel",
              # the waveform losses: four fp64 accumulators per lane
              "waveloss.hip": "wave_loss_",
              # the ESTOI segment kernel holds a 30-frame row, then two 15-band columns, of fp64 per lane
              # (the STOI criterion's backward kernels: the segment kernel holds two 30-frame rows of fp64 per lane)
              "stoi.hip": ("estoi_", "stoi_loss_"),
              # the mixer's sample passes hold four quads and an fp64 accumulator per lane; its gain kernel calls pow
              "mix.hip": "mix_",
              # the reverberator holds 8 outputs, their early parts, 16 samples and 8 taps per lane
              "reverb.hip": "reverb_",
              # the resampler's chain is an fp64 accumulator and two LDS pointers per lane
              "resample.hip": "resample_"}


def _check_no_scratch(src, remarks):
    """remarks: the compiler's stderr of `src`.  Raises if a NO_SCRATCH kernel uses scratch (or none was seen)."""
    wants = NO_SCRATCH[os.path.basename(src)]
    wants = (wants,) if isinstance(wants, str) else wants
    seen, name = dict.fromkeys(wants, 0), None
    for line in remarks.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)", line)
        for want in wants:
            if m and name and want in name:
                seen[want] += 1
                if int(m.group(1)) != 0:
                    raise RuntimeError("%s: kernel %s uses %s bytes of scratch per lane" % (src, name, m.group(1)))
    for want in wants:
        if not seen[want]:
            raise RuntimeError("%s: no resource-usage remark for %s" % (src, want))


def _sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")))


def _deps():
    return _sources() + glob.glob(os.path.join(CSRC, "*.h")) + \
        [os.path.join(os.path.dirname(HERE), "include", n) for n in ("drnmf.h", "drnmf_lstm.h", "drnmf_score.h", "drnmf_enhance.h", "drnmf_sdr.h",
                                                                     "drnmf_dataset.h", "drnmf_stream.h", "drnmf_snmf.h", "drnmf_snmf_f16.h",
                                                                     "drnmf_target.h", "drnmf_estoi.h", "drnmf_snmf_adapt.h",
                                                                     "drnmf_snmf_kl.h", "drnmf_snmf_online.h", "drnmf_mix.h",
                                                                     "drnmf_waveloss.h", "drnmf_reverb.h", "drnmf_stoi_loss.h",
                                                                     "drnmf_resample.h")] + \
        [os.path.abspath(__file__)]


STAMP = LIB + ".srchash"


def _src_hash():
    """Content hash of everything the library is built from (mtimes do not survive the copy to the
    GPU box in any particular order)."""
    h = hashlib.sha256(" ".join(FLAGS).encode())
    for p in sorted(_deps()):
        h.update(os.path.basename(p).encode())
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def needs_build():
    if not os.path.exists(LIB) or not os.path.exists(STAMP):
        return True
    with open(STAMP) as f:
        return f.read().strip() != _src_hash()


def build(force=False, verbose=True):
    if not force and not needs_build():
        return LIB
    # one builder at a time: `bench.py --gpus N` starts N processes that all call build()
    with open(LIB + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and not needs_build():     # another process built it meanwhile
                return LIB
            return _build_locked(force, verbose)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def _build_locked(force, verbose):
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    objs, procs = [], []
    for src in _sources():
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        objs.append(obj)
        # per-object stamp: this source + every header + the flags
        hh = hashlib.sha256(" ".join(FLAGS).encode())
        for p in sorted(q for q in _deps() if not q.endswith(".hip") or q == src):
            with open(p, "rb") as f:
                hh.update(f.read())
        want = hh.hexdigest()
        stamp = obj + ".srchash"
        if not force and os.path.exists(obj) and os.path.exists(stamp):
            with open(stamp) as f:
                if f.read().strip() == want:
                    continue
        cmd = [HIPCC] + FLAGS + ["-c", src, "-o", obj]
        log = None
        if os.path.basename(src) in NO_SCRATCH:
            cmd.insert(-4, "-Rpass-analysis=kernel-resource-usage")
            log = open(obj + ".remarks", "w+")
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((src, stamp, want, subprocess.Popen(cmd, stderr=log), log))
    for src, stamp, want, p, log in procs:
        rc = p.wait()
        if log is not None:
            log.seek(0)
            remarks = log.read()
            log.close()
            if rc != 0 or re.search(r"(warning|error):", remarks):       # as without the flag: show them
                print(remarks, file=sys.stderr, flush=True)
        if rc != 0:
            raise RuntimeError("hipcc failed on %s" % src)
        if log is not None:
            _check_no_scratch(src, remarks)
        with open(stamp, "w") as f:
            f.write(want + "\n")
    tmp = LIB + ".tmp.%d" % os.getpid()
    cmd = [HIPCC] + ARCH + ["-shared", "-fPIC", "-o", tmp] + objs + ["-ldl"]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    os.replace(tmp, LIB)            # a process that already mapped the old file keeps it
    with open(STAMP, "w") as f:
        f.write(_src_hash() + "\n")
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)
