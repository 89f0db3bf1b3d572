"""Build libvamp_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "vamp_hip.hip")
OUT = os.path.join(HERE, "libvamp_hip.so")
# every file vamp_hip.hip #includes: a regenerated matrix or an edited header must trigger a rebuild
DEPS = [SRC] + [os.path.join(HERE, "csrc", f) for f in ("ff_matrix.inc", "ff_matrix32.inc", "voigt_math.hpp", "map_search.hpp", "host_plan.hpp",
                                                         "abi_state.hpp", "draws.hpp", "ff_predicates.hpp", "ff_moments.hpp", "ff_super.inc")
                if os.path.exists(os.path.join(HERE, "csrc", f))] + [os.path.join(HERE, "..", "include", "vamp_hip.h")]


# -fno-slp-vectorize: left to itself the SLP vectoriser pairs the independent fp32 chains of a lane's four pixels
# into v_pk_fma_f32 / v_pk_mul_f32 and pays for the register pairing with v_mov (429 packed + 464 moves in the fp32
# headline kernel).  On gfx950 a packed fp32 instruction issues no faster than its two halves, so this is pure
# overhead: 2.699 -> 2.220 ms per half-step on the fp32 headline, fp64 unchanged (3.251 -> 3.239)
# (profiles/r03_b_f32_variants.txt; MI355X_MICROARCH.md lists packed fp32 VALU as an anti-lever).
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-shared", "-fPIC"]

# The side libraries share their flags, the frame of their entry points (side_call.hpp) and -- all but the
# diagnostics -- the lane-group evaluator (lane_group.hpp); the posterior, the predictive density and PSIS-LOO also the
# chain checks and the pass planner (chain_groups.hpp), the predictive density and PSIS-LOO the pointwise
# log-likelihood stage (pointwise_ll.hpp): an edit of a shared header rebuilds what includes it
SIDE_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-fvisibility=hidden"]
POST_FLAGS = EVID_FLAGS = PRED_FLAGS = LOO_FLAGS = RELABEL_FLAGS = FISHER_FLAGS = LAPLACE_FLAGS = HMC_FLAGS = METRIC_FLAGS = SIDE_FLAGS      # (names the tests of those libraries read)
SIDE_CALL = os.path.join(HERE, "csrc", "side_call.hpp")
LANE_GROUP = os.path.join(HERE, "csrc", "lane_group.hpp")
CHAIN_GROUPS = os.path.join(HERE, "csrc", "chain_groups.hpp")
POINTWISE_LL = os.path.join(HERE, "csrc", "pointwise_ll.hpp")

# libvamp_diag.so (include/vamp_diag.h): the chain diagnostics, a library of its own with its own dependency list,
# so that an edit of chain_diag.hip rebuilds it in seconds and leaves the main library alone
DIAG_SRC = os.path.join(HERE, "csrc", "chain_diag.hip")
DIAG_OUT = os.path.join(HERE, "libvamp_diag.so")
DIAG_DEPS = [DIAG_SRC, SIDE_CALL, os.path.join(HERE, "..", "include", "vamp_diag.h")]

# libvamp_post.so (include/vamp_post.h): the posterior summaries, a third library on the same terms; it shares
# voigt_math.hpp with the main library, so an edit of the evaluator rebuilds both
POST_SRC = os.path.join(HERE, "csrc", "posterior.hip")
POST_OUT = os.path.join(HERE, "libvamp_post.so")
POST_DEPS = [POST_SRC, SIDE_CALL, LANE_GROUP, CHAIN_GROUPS, os.path.join(HERE, "csrc", "voigt_math.hpp"),
             os.path.join(HERE, "..", "include", "vamp_post.h")]

# libvamp_evid.so (include/vamp_evid.h): the log-evidence from tempered ensembles, a fourth library on the same terms;
# it shares the evaluator (voigt_math.hpp) and the draws (draws.hpp) with the main library
EVID_SRC = os.path.join(HERE, "csrc", "evidence.hip")
EVID_OUT = os.path.join(HERE, "libvamp_evid.so")
EVID_DEPS = [EVID_SRC, SIDE_CALL, LANE_GROUP, os.path.join(HERE, "csrc", "voigt_math.hpp"), os.path.join(HERE, "csrc", "draws.hpp"),
             os.path.join(HERE, "..", "include", "vamp_evid.h")]

# libvamp_pred.so (include/vamp_pred.h): the pointwise predictive density and WAIC, a fifth library on the same terms;
# it shares the evaluator (voigt_math.hpp) with the main library
PRED_SRC = os.path.join(HERE, "csrc", "predictive.hip")
PRED_OUT = os.path.join(HERE, "libvamp_pred.so")
PRED_DEPS = [PRED_SRC, SIDE_CALL, LANE_GROUP, CHAIN_GROUPS, POINTWISE_LL, os.path.join(HERE, "csrc", "voigt_math.hpp"),
             os.path.join(HERE, "..", "include", "vamp_pred.h")]

# libvamp_loo.so (include/vamp_loo.h): PSIS-LOO, a sixth library on the same terms; it evaluates the log-likelihood
# with the predictive library's stage, so it shares the evaluator (voigt_math.hpp) with the main library too
LOO_SRC = os.path.join(HERE, "csrc", "loo.hip")
LOO_OUT = os.path.join(HERE, "libvamp_loo.so")
LOO_DEPS = [LOO_SRC, SIDE_CALL, LANE_GROUP, CHAIN_GROUPS, POINTWISE_LL, os.path.join(HERE, "csrc", "voigt_math.hpp"),
            os.path.join(HERE, "..", "include", "vamp_loo.h")]

# libvamp_relabel.so (include/vamp_relabel.h): the relabelling that undoes label switching, a seventh library on the
# same terms; it moves parameters and evaluates nothing, so it shares only the call frame
RELABEL_SRC = os.path.join(HERE, "csrc", "relabel.hip")
RELABEL_OUT = os.path.join(HERE, "libvamp_relabel.so")
RELABEL_DEPS = [RELABEL_SRC, SIDE_CALL, os.path.join(HERE, "csrc", "relabel_host.hpp"), os.path.join(HERE, "..", "include", "vamp_relabel.h")]

# libvamp_fisher.so (include/vamp_fisher.h): gradient, information matrix and covariance at given points from the
# analytic Jacobian, an eighth library on the same terms; it shares the evaluator (voigt_math.hpp) with the main library
# and adds the derivative evaluator (voigt_grad.hpp)
FISHER_SRC = os.path.join(HERE, "csrc", "fisher.hip")
FISHER_OUT = os.path.join(HERE, "libvamp_fisher.so")
FISHER_DEPS = [FISHER_SRC, SIDE_CALL, LANE_GROUP, os.path.join(HERE, "csrc", "voigt_math.hpp"), os.path.join(HERE, "csrc", "voigt_grad.hpp"),
               os.path.join(HERE, "..", "include", "vamp_fisher.h")]

# libvamp_laplace.so (include/vamp_laplace.h): importance sampling from a Gaussian proposal, a ninth library on the same
# terms; it shares the evaluator (voigt_math.hpp) and the draws (draws.hpp) with the main library
LAPLACE_SRC = os.path.join(HERE, "csrc", "laplace.hip")
LAPLACE_OUT = os.path.join(HERE, "libvamp_laplace.so")
LAPLACE_DEPS = [LAPLACE_SRC, SIDE_CALL, LANE_GROUP, os.path.join(HERE, "csrc", "voigt_math.hpp"), os.path.join(HERE, "csrc", "draws.hpp"),
                os.path.join(HERE, "..", "include", "vamp_laplace.h")]

# libvamp_hmc.so (include/vamp_hmc.h): preconditioned Hamiltonian Monte Carlo chains per region, a tenth library on the
# same terms; it shares the evaluator (voigt_math.hpp), the derivative evaluator (voigt_grad.hpp) and Philox (draws.hpp)
HMC_SRC = os.path.join(HERE, "csrc", "hmc.hip")
HMC_OUT = os.path.join(HERE, "libvamp_hmc.so")
HMC_DEPS = [HMC_SRC, SIDE_CALL, LANE_GROUP, os.path.join(HERE, "csrc", "voigt_math.hpp"), os.path.join(HERE, "csrc", "voigt_grad.hpp"),
            os.path.join(HERE, "csrc", "draws.hpp"), os.path.join(HERE, "..", "include", "vamp_hmc.h")]

# libvamp_metric.so (include/vamp_metric.h): a positive-definite metric from any symmetric matrix, an eleventh library on
# the same terms; it never sees parameters or data, so it shares the call frame and lane_group.hpp's lds_fence() only;
# its host-side checks and launch plan are a plain C++ header (tests/host/metric_host.cpp)
METRIC_SRC = os.path.join(HERE, "csrc", "metric.hip")
METRIC_OUT = os.path.join(HERE, "libvamp_metric.so")
METRIC_DEPS = [METRIC_SRC, SIDE_CALL, LANE_GROUP, os.path.join(HERE, "csrc", "voigt_math.hpp"), os.path.join(HERE, "csrc", "metric_host.hpp"),
               os.path.join(HERE, "..", "include", "vamp_metric.h")]


def _compile(out, src, deps, flags, force, verbose):
    if not force and os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + flags + ["-o", out, src]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return out


def build_diag(force=False, verbose=True):
    """libvamp_diag.so; returns its path"""
    return _compile(DIAG_OUT, DIAG_SRC, DIAG_DEPS, SIDE_FLAGS, force, verbose)


def build_post(force=False, verbose=True, out=None, defines=()):
    """libvamp_post.so; returns its path.  ``out`` / ``defines``: a variant build beside it (tools/bench_post.py
    compares the orientations of the scratch and the 16-lane form)."""
    return _compile(out or POST_OUT, POST_SRC, POST_DEPS, SIDE_FLAGS + ["-D" + d for d in defines], force, verbose)


def build_evid(force=False, verbose=True, out=None, defines=()):
    """libvamp_evid.so; returns its path.  ``out`` / ``defines``: a variant build beside it (tools/bench_evid.py
    compares the lane widths)."""
    return _compile(out or EVID_OUT, EVID_SRC, EVID_DEPS, SIDE_FLAGS + ["-D" + d for d in defines], force, verbose)


def build_pred(force=False, verbose=True, out=None, defines=()):
    """libvamp_pred.so; returns its path.  ``out`` / ``defines``: a variant build beside it (tools/bench_pred.py
    compares the orientations of the scratch and the 16-lane form)."""
    return _compile(out or PRED_OUT, PRED_SRC, PRED_DEPS, SIDE_FLAGS + ["-D" + d for d in defines], force, verbose)


def build_loo(force=False, verbose=True, out=None, defines=()):
    """libvamp_loo.so; returns its path.  ``out`` / ``defines``: a variant build beside it"""
    return _compile(out or LOO_OUT, LOO_SRC, LOO_DEPS, SIDE_FLAGS + ["-D" + d for d in defines], force, verbose)


def build_relabel(force=False, verbose=True, out=None, defines=()):
    """libvamp_relabel.so; returns its path.  ``out`` / ``defines``: a variant build beside it"""
    return _compile(out or RELABEL_OUT, RELABEL_SRC, RELABEL_DEPS, SIDE_FLAGS + ["-D" + d for d in defines], force, verbose)


def build_fisher(force=False, verbose=True, out=None, defines=()):
    """libvamp_fisher.so; returns its path.  ``out`` / ``defines``: a variant build beside it"""
    return _compile(out or FISHER_OUT, FISHER_SRC, FISHER_DEPS, SIDE_FLAGS + ["-D" + d for d in defines], force, verbose)


def build_laplace(force=False, verbose=True, out=None, defines=()):
    """libvamp_laplace.so; returns its path.  ``out`` / ``defines``: a variant build beside it (tools/bench_laplace.py
    compares the lane widths)."""
    return _compile(out or LAPLACE_OUT, LAPLACE_SRC, LAPLACE_DEPS, SIDE_FLAGS + ["-D" + d for d in defines], force, verbose)


def build_hmc(force=False, verbose=True, out=None, defines=()):
    """libvamp_hmc.so; returns its path.  ``out`` / ``defines``: a variant build beside it (tools/bench_hmc.py compares
    the two reductions of the gradient)."""
    return _compile(out or HMC_OUT, HMC_SRC, HMC_DEPS, SIDE_FLAGS + ["-D" + d for d in defines], force, verbose)


def build_metric(force=False, verbose=True, out=None, defines=()):
    """libvamp_metric.so; returns its path.  ``out`` / ``defines``: a variant build beside it"""
    return _compile(out or METRIC_OUT, METRIC_SRC, METRIC_DEPS, SIDE_FLAGS + ["-D" + d for d in defines], force, verbose)


def build(force=False, verbose=True):
    """The eleven libraries; returns the path of libvamp_hip.so (tests/test_abi.py binds what this returns)."""
    build_diag(force=force, verbose=verbose)
    build_post(force=force, verbose=verbose)
    build_evid(force=force, verbose=verbose)
    build_pred(force=force, verbose=verbose)
    build_loo(force=force, verbose=verbose)
    build_relabel(force=force, verbose=verbose)
    build_fisher(force=force, verbose=verbose)
    build_laplace(force=force, verbose=verbose)
    build_hmc(force=force, verbose=verbose)
    build_metric(force=force, verbose=verbose)
    return _compile(OUT, SRC, DEPS, FLAGS, force, verbose)


if __name__ == "__main__":
    build(force="--force" in sys.argv)
