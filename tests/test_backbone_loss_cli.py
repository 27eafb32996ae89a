"""What `--backbone_loss` needs without a GPU: the flag on the command line, the new entry points in header, exports and ctypes
table, their host-side argument checks and workspace sizing, and the host mirror's signatures."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ptamd_nerf_bb_fwd", "ptamd_nerf_bb_bwd", "ptamd_drmsd_bb_workspace_bytes", "ptamd_drmsd_bb_workspace_bytes_budget",
       "ptamd_drmsd_bb_fwd_bwd", "ptamd_drmsd_bb_fwd_bwd_budget")


@pytest.fixture(scope="module")
def built_lib():
    from protein_transformer_amd import _lib, build
    build.build()                       # hipcc cross-compiles gfx950 without a GPU
    return _lib


def test_parser_accepts_the_flag():
    from protein_transformer_amd.train import create_parser
    assert create_parser().parse_args([]).backbone_loss is False
    for loss in ("drmsd", "lndrmsd", "combined", "mse"):
        a = create_parser().parse_args(["--backbone_loss", "-l", loss])
        assert a.backbone_loss is True and a.loss == loss


def test_entry_points_in_header_exports_and_table(built_lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptamd.h")).read(), flags=re.S)
    handle = ctypes.CDLL(built_lib.LIB_PATH)
    built_lib.lib()
    assert not built_lib.MISSING
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert hasattr(handle, name), name
        assert name in built_lib.SIGNATURES, name
    # same argument lists as the full-atom pair sweep: a caller switches by name
    for a, b in (("ptamd_drmsd_bb_fwd_bwd", "ptamd_drmsd_fwd_bwd"), ("ptamd_drmsd_bb_fwd_bwd_budget", "ptamd_drmsd_fwd_bwd_budget"),
                 ("ptamd_drmsd_bb_workspace_bytes", "ptamd_drmsd_workspace_bytes"), ("ptamd_nerf_bb_fwd", "ptamd_nerf_fwd")):
        assert built_lib.SIGNATURES[a] == built_lib.SIGNATURES[b]


def test_host_side_checks_and_sizing(built_lib):
    lib = built_lib.lib()
    full, bb = lib.ptamd_drmsd_workspace_bytes(32, 512), lib.ptamd_drmsd_bb_workspace_bytes(32, 512)
    assert 0 < bb < full and 3 * bb < full                      # sized from 3 L atoms per protein, not 14 L
    assert bb > 32 * 512 * 3 * 52                                # 52 B per atom of compacted copies + the partial sums
    assert lib.ptamd_drmsd_bb_workspace_bytes_budget(32, 512, 0) == bb
    assert lib.ptamd_drmsd_bb_workspace_bytes(0, 512) == 0
    assert lib.ptamd_drmsd_bb_workspace_bytes(32, 1500) < lib.ptamd_drmsd_workspace_bytes(32, 1500)
    # the full-atom sizes are what they were
    assert full > 32 * 512 * 14 * 52 and full <= 200 << 20
    # argument validation happens on the host, before any launch
    assert lib.ptamd_nerf_bb_fwd(None, None, 0, 5, None, None, None) == -1               # PTAMD_ERR_BAD_SHAPE
    assert lib.ptamd_nerf_bb_fwd(None, None, 2, 5000, None, None, None) == -2            # PTAMD_ERR_TOO_LONG
    assert lib.ptamd_nerf_bb_bwd(None, None, None, None, 2, 0, None, None) == -1
    assert lib.ptamd_nerf_bb_bwd(None, None, None, None, 2, 5000, None, None) == -2
    assert lib.ptamd_drmsd_bb_fwd_bwd(None, None, None, 2, 8, None, None, None, 0, None) == -3      # PTAMD_ERR_WORKSPACE
    assert lib.ptamd_drmsd_bb_fwd_bwd(None, None, None, 0, 8, None, None, None, 0, None) == -1


def test_host_mirror_signatures_and_no_cpu_path(built_lib):
    from protein_transformer_amd import losses, train
    from protein_transformer_amd.protein import Structure
    for fn in (Structure.nerf_forward, Structure.nerf_backward, losses.drmsd_forward_backward, losses.batch_loss,
               losses.compute_batch_drmsd, losses.drmsd_work):
        p = inspect.signature(fn).parameters["backbone_only"]
        assert p.default is False, fn
    for mod in (losses, train):
        assert "NotImplementedError(\"--backbone_loss" not in inspect.getsource(mod)
    with pytest.raises(RuntimeError, match="device tensors only"):
        Structure.nerf_forward(torch.zeros(1, 3, 12), torch.zeros(1, 3, dtype=torch.int64), backbone_only=True)
    with pytest.raises(RuntimeError, match="device tensors only"):
        losses.drmsd_forward_backward(torch.zeros(1, 6, 3), torch.zeros(1, 28, 3), torch.zeros(1, 2, dtype=torch.int64),
                                      backbone_only=True)
