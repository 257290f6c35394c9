"""In-tree build of libicp_mi355x.so (HIP kernels + C ABI) for gfx950."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(_HERE, "libicp_mi355x.so")
_SOURCES = ["capi.hip", "sort.hip", "kernels.h", "device_math.h", "list_reuse.h", "loop_plan.h", "workspace_layout.h", "nn_mfma.h", "icp_small.h", "icp_small_kernel.inc", "icp_gated.h", "icp_robust.h", "icp_gicp.h", "icp_gicp_row.inc", "knn_lists.h", "nn_bounded.h", "solo_pass.h", "nn_culled.h", "voxel.h", "scan_context.h", "occupancy.h", "global_map.h", "raycast.h", "raycount.h", "live_plane.h", "live_counts.h", "ground.h", "static_map.h", "deskew.h", "deskew_host.h", "loop_store.h", "se3.h", "pose_graph.h", "pose_graph_loss.h", "pose_graph_info.h", "pose_graph_info_host.h", "pose_graph_marginals.h", "pose_graph_marginals_host.h", "local_map.h", "Makefile"]


def _stale():
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    deps = [os.path.join(CSRC, s) for s in _SOURCES]
    deps.append(os.path.join(_HERE, "..", "include", "icp_mi355x.h"))
    return any(os.path.exists(d) and os.path.getmtime(d) > t for d in deps)


def build_library(force=False, verbose=False):
    """Compile with hipcc --offload-arch=gfx950 (cross-compiles without a GPU)."""
    if force or _stale():
        cmd = ["make", "-C", CSRC, "OUT=" + LIB_PATH]
        if force:
            cmd.insert(1, "-B")
        out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if verbose or out.returncode != 0:
            print(out.stdout)
        if out.returncode != 0:
            raise RuntimeError("hipcc build of libicp_mi355x.so failed")
    return LIB_PATH
