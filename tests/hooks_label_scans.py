"""Test infrastructure: the test hook of the scans' labelling (erasor_hip_debug_ls_effort), called through the hooks build of the library
as tests/hooks.py calls the others (inside hooks.hooks_library())."""
import ctypes as C

import numpy as np

import erasor_amd


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def debug_ls_effort(g, tree, queries, tau):
    """label_scans' bounded search (k_ls_query's static pass, one frame, identity transforms) of `queries` over the tree of `tree`:
    "codes" (0: a tree point within tau, else 1) and "effort", effort[i] = (leaves opened, leaf points tested) of query i -- the
    counterpart of hooks.debug_nn_effort(g, tree, queries, False) on the same input"""
    tree = np.ascontiguousarray(tree, np.float32).reshape(-1, 4)
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, 4)
    codes, effort = np.zeros(len(q), np.uint8), np.zeros((len(q), 2), np.uint32)
    g._check(erasor_amd.lib().erasor_hip_debug_ls_effort(g._h, _p(tree), C.c_size_t(len(tree)), _p(q), C.c_size_t(len(q)), C.c_double(tau),
                                                         _p(codes), _p(effort)))
    return {"codes": codes, "effort": effort}
