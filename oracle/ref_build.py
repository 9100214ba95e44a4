"""Recipe: compile the reference's own CUDA kernels for gfx950 (test infrastructure only).

The reference implements NMS, RoIAlign, RoIPool and the RoI crop sampler only as CUDA
extensions.  Their four kernel files use nothing but the CUDA runtime API (the TH/THC glue
lives in the ``*_cuda.c`` wrappers, which are not needed), so hipcc compiles them unchanged
once ``oracle/ref_cuda_shim.h`` maps the runtime names.  The sources are read straight from the
reference checkout; nothing of them is copied into this repository, and the products land
in ``oracle/_ref/`` (ignored by git):

  libtlod_ref.so      -ffp-contract=off, -O2, hipcc's default (correctly rounded) f32 division
                      and no fast-math: the arithmetic oracle/{nms,roi}.py and the HIP
                      kernels restate.
  libtlod_ref_fma.so  the same with hipcc's default contraction (nvcc contracts by default);
                      only the contraction test of tests/test_reference_kernels_gpu.py uses it.

Entry points (all ``extern "C"``): nms_cuda_compute (nms_cuda_kernel.cu:87),
ROIAlignForwardLaucher / ROIAlignBackwardLaucher (roi_align_kernel.cu:73, :145),
ROIPoolForwardLaucher / ROIPoolBackwardLaucher (roi_pooling_kernel.cu:95, :205, declared
extern "C" by roi_pooling_kernel.h), BilinearSamplerBHWD_updateOutput_cuda_kernel /
BilinearSamplerBHWD_updateGradInput_cuda_kernel (roi_crop_cuda_kernel.cu:201, :257).
oracle/ref_kernels.py wraps them.
"""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEFAULT_OUT = os.path.join(HERE, "_ref")
SHIM = os.path.join(HERE, "ref_cuda_shim.h")
ENV = "TLOD_REFERENCE_DIR"
ARCH = "gfx950"
MAX_JOBS = 16

SOURCES = (
    "lib/model/nms/src/nms_cuda_kernel.cu",
    "lib/model/roi_align/src/roi_align_kernel.cu",
    "lib/model/roi_pooling/src/roi_pooling_kernel.cu",
    "lib/model/roi_crop/src/roi_crop_cuda_kernel.cu",
)
SYMBOLS = (
    "nms_cuda_compute",
    "ROIAlignForwardLaucher",
    "ROIAlignBackwardLaucher",
    "ROIPoolForwardLaucher",
    "ROIPoolBackwardLaucher",
    "BilinearSamplerBHWD_updateOutput_cuda_kernel",
    "BilinearSamplerBHWD_updateGradInput_cuda_kernel",
)
# library name -> extra compile flags ([] = hipcc's default -ffp-contract)
VARIANTS = {
    "libtlod_ref.so": ["-ffp-contract=off"],
    "libtlod_ref_fma.so": [],
}


def hipcc():
    return os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def find_reference():
    """The reference checkout: $TLOD_REFERENCE_DIR, else a ``reference`` directory beside the
    repository root.  None when neither holds all four kernel files."""
    for cand in (os.environ.get(ENV), os.path.join(os.path.dirname(ROOT), "reference")):
        if cand and all(os.path.isfile(os.path.join(cand, s)) for s in SOURCES):
            return os.path.abspath(cand)
    return None


def _inputs(ref_dir):
    files = [SHIM, os.path.abspath(__file__)]
    for s in SOURCES:
        src = os.path.join(ref_dir, s)
        files.append(src)
        hdr = os.path.splitext(src)[0] + ".h"
        if os.path.isfile(hdr):
            files.append(hdr)
    return files


def up_to_date(ref_dir, out_dir=DEFAULT_OUT):
    outs = [os.path.join(out_dir, n) for n in VARIANTS]
    if not all(os.path.isfile(o) for o in outs):
        return False
    return min(os.path.getmtime(o) for o in outs) > max(os.path.getmtime(f) for f in _inputs(ref_dir))


def build_reference(ref_dir, out_dir=DEFAULT_OUT, jobs=MAX_JOBS):
    """Compile the four kernel files from ``ref_dir`` into out_dir/libtlod_ref{,_fma}.so.
    Returns the list of libraries built ([] when they were already newer than the sources, the
    shim and this recipe)."""
    ref_dir = os.path.abspath(ref_dir)
    missing = [s for s in SOURCES if not os.path.isfile(os.path.join(ref_dir, s))]
    if missing:
        raise FileNotFoundError(f"not a reference checkout ({ref_dir}): missing {missing}")
    if up_to_date(ref_dir, out_dir):
        return []
    cc = hipcc()
    os.makedirs(out_dir, exist_ok=True)
    for libname in VARIANTS:  # a failed rebuild must not leave the previous libraries behind
        if os.path.exists(os.path.join(out_dir, libname)):
            os.remove(os.path.join(out_dir, libname))
    units = []  # (library, object, command)
    objdirs = []
    for libname, extra in VARIANTS.items():
        tag = os.path.splitext(libname)[0]
        objdir = os.path.join(out_dir, "obj_" + tag)
        shutil.rmtree(objdir, ignore_errors=True)
        os.makedirs(objdir)
        objdirs.append(objdir)
        for s in SOURCES:
            src = os.path.join(ref_dir, s)
            obj = os.path.join(objdir, os.path.splitext(os.path.basename(s))[0] + ".o")
            cmd = [cc, f"--offload-arch={ARCH}", "-x", "hip", "-O2", "-fPIC", *extra,
                   "-w", "-include", SHIM, "-I", os.path.dirname(src), "-c", src, "-o", obj]
            units.append((libname, obj, cmd))

    def compile_one(u):
        subprocess.run(u[2], check=True)

    with ThreadPoolExecutor(max_workers=max(1, min(int(jobs), MAX_JOBS, len(units)))) as ex:
        list(ex.map(compile_one, units))
    built = []
    for libname in VARIANTS:
        objs = [o for (n, o, _) in units if n == libname]
        out = os.path.join(out_dir, libname)
        subprocess.run([cc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", out, *objs],
                       check=True)
        built.append(out)
    for objdir in objdirs:  # the libraries are the product; the objects are not kept
        shutil.rmtree(objdir, ignore_errors=True)
    return built


def build_if_reference_present(out_dir=None):
    """build()'s hook: compile when a checkout is found, otherwise say so in one line.
    ``out_dir`` defaults to DEFAULT_OUT, read at call time."""
    ref_dir = find_reference()
    if ref_dir is None:
        print(f"oracle/_ref: no reference checkout (${ENV} unset, no ../reference): "
              "reference-kernel tests will skip")
        return []
    return build_reference(ref_dir, DEFAULT_OUT if out_dir is None else out_dir)


if __name__ == "__main__":
    print(build_if_reference_present())
