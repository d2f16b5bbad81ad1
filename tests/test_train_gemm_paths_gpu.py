"""Every path of the training step's matrix products against float64 (the walk of tests/train_gemm_paths.py): vh_linear_ex on
both operand stagings, every epilogue body and the tail split's fix-up; vh_gemm_tn on every ending of its schedule and every
slice plan; vh_transpose / TransposePlan; vh_gemm_batched on float data, split and unsplit.

Each case: the result within min(SUM_MARGIN x written figure, 1) x the derived cap of float64 (a NaN fails), the integer flavour
exact wherever the epilogue is arithmetic only (its transcendental outputs: within the cap), a second launch bit-identical
(column sums and the split vh_gemm_batched use atomics: the bound only).  Workspaces are handed over through the ctypes entries
at exactly *_ws_bytes bytes and full of NaN; outputs sit in larger buffers full of a sentinel that rows >= M and columns >= N
must keep; operand padding beyond the 4-column pad holds NaN.

The written figures below are the worst error, in units of the derived cap, that fp32 arithmetic has on the CPU (plain torch,
the 32-wide-slab order with the slices added in slice order, and one FMA chain over k on a sample of rows) -- re-measured by
tests/test_train_gemm_paths_cpu.py, never taken from a kernel run."""
import ctypes as C

import pytest
import torch

from tests import train_gemm_paths as P

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENT = P.SENTINEL

# figure key -> written figures of (out, pre_out, colsum); None where the case has no such output
LIN_FP32_ERR = {
    '129x256x64-bias': (0.064, None, None),
    '129x256x64-res': (0.052, None, None),
    '129x256x64-gelu_pre': (0.057, 0.064, None),
    '129x256x64-gelu_res': (0.058, None, None),
    '129x256x64-gelu_d': (0.057, 0.04, None),
    '129x256x64-gelu_bwd': (0.064, None, None),
    '129x256x64-mul': (0.079, None, None),
    '129x256x64-res_cs': (0.052, None, 0.012),
    '129x256x64-gelu_d_cs': (0.057, 0.04, 0.011),
    '129x256x64-drop_res': (0.053, None, None),
    '129x256x64-drop_gelu': (0.055, 0.064, None),
    '129x256x64-drop_gelu_d': (0.064, 0.041, None),
    '129x256x64-drop_res_cs': (0.053, None, 0.013),
    '129x128x1056-bias': (0.0046, None, None),
    '129x128x1056-res': (0.0046, None, None),
    '129x128x1056-gelu_pre': (0.0033, 0.0046, None),
    '129x128x1056-gelu_res': (0.0032, None, None),
    '129x128x1056-gelu_d': (0.0033, 0.0022, None),
    '129x128x1056-gelu_bwd': (0.0042, None, None),
    '129x128x1056-mul': (0.0049, None, None),
    '129x128x1056-res_cs': (0.0046, None, 0.00062),
    '129x128x1056-gelu_d_cs': (0.0033, 0.0022, 0.00049),
    '129x128x1056-drop_res': (0.0037, None, None),
    '129x128x1056-drop_gelu': (0.0033, 0.0046, None),
    '129x128x1056-drop_gelu_d': (0.0033, 0.0022, None),
    '129x128x1056-drop_res_cs': (0.0037, None, 0.00053),
    '5x128x32-gelu_pre': (0.048, 0.06, None),
    '5x128x32-gelu_d': (0.048, 0.032, None),
    '5x128x32-gelu_bwd': (0.068, None, None),
    '5x128x32-mul': (0.08, None, None),
    '5x128x32-res_cs': (0.061, None, 0.044),
    '5x128x32-gelu_d_cs': (0.048, 0.032, 0.023),
    '5x128x32-drop_res': (0.065, None, None),
    '5x128x32-drop_gelu': (0.053, 0.06, None),
    '5x128x32-drop_gelu_d': (0.051, 0.035, None),
    '5x128x32-drop_res_cs': (0.065, None, 0.054),
    '130x1025x64-bias': (0.079, None, None),
    '130x1025x64-res': (0.082, None, None),
    '130x1025x64-gelu_pre': (0.055, 0.079, None),
    '130x1025x64-gelu_res': (0.063, None, None),
    '130x1025x64-gelu_d': (0.055, 0.042, None),
    '130x1025x64-gelu_bwd': (0.066, None, None),
    '130x1025x64-mul': (0.092, None, None),
    '2176x2048x256-bias': (0.024, None, None),
    '2176x2048x256-res': (0.024, None, None),
    '2176x2048x256-gelu_pre': (0.019, 0.024, None),
    '2176x2048x256-gelu_res': (0.019, None, None),
    '2176x2048x256-gelu_d': (0.019, 0.023, None),
    '2176x2048x256-gelu_bwd': (0.027, None, None),
    '2176x2048x256-mul': (0.03, None, None),
    '2176x2048x256-res_cs': (0.024, None, 0.0016),
    '2176x2048x256-gelu_d_cs': (0.019, 0.023, 0.0016),
    '2176x2048x256-drop_res': (0.024, None, None),
    '2176x2048x256-drop_gelu': (0.02, 0.024, None),
    '2176x2048x256-drop_gelu_d': (0.019, 0.023, None),
    '2176x2048x256-drop_res_cs': (0.024, None, 0.0016),
    '3072x2048x256-bias': (0.024, None, None),
    '3072x2048x256-res': (0.024, None, None),
    '3072x2048x256-gelu_pre': (0.021, 0.024, None),
    '3072x2048x256-gelu_res': (0.021, None, None),
    '3072x2048x256-gelu_d': (0.021, 0.022, None),
    '3072x2048x256-gelu_bwd': (0.025, None, None),
    '3072x2048x256-mul': (0.028, None, None),
    '3072x2048x256-res_cs': (0.024, None, 0.0013),
    '3072x2048x256-gelu_d_cs': (0.021, 0.022, 0.0011),
    '3072x2048x256-drop_res': (0.025, None, None),
    '3072x2048x256-drop_gelu': (0.022, 0.024, None),
    '3072x2048x256-drop_gelu_d': (0.022, 0.019, None),
    '3072x2048x256-drop_res_cs': (0.025, None, 0.0013),
    '2176x2048x384-bias': (0.016, None, None),
    '2176x2048x384-res': (0.016, None, None),
    '2176x2048x384-gelu_pre': (0.014, 0.016, None),
    '2176x2048x384-gelu_res': (0.014, None, None),
    '2176x2048x384-gelu_d': (0.014, 0.012, None),
    '2176x2048x384-gelu_bwd': (0.017, None, None),
    '2176x2048x384-mul': (0.018, None, None),
    '2176x2048x384-res_cs': (0.016, None, 0.0013),
    '2176x2048x384-gelu_d_cs': (0.014, 0.012, 0.0012),
    '2176x2048x384-drop_res': (0.017, None, None),
    '2176x2048x384-drop_gelu': (0.015, 0.016, None),
    '2176x2048x384-drop_gelu_d': (0.014, 0.012, None),
    '2176x2048x384-drop_res_cs': (0.017, None, 0.0013),
    '2176x2048x1024-bias': (0.0056, None, None),
    '2176x2048x1024-res': (0.0056, None, None),
    '2176x2048x1024-gelu_pre': (0.0051, 0.0056, None),
    '2176x2048x1024-gelu_res': (0.0051, None, None),
    '2176x2048x1024-gelu_d': (0.0051, 0.0037, None),
    '2176x2048x1024-gelu_bwd': (0.0051, None, None),
    '2176x2048x1024-mul': (0.0059, None, None),
    '2176x2048x1024-res_cs': (0.0056, None, 0.00075),
    '2176x2048x1024-gelu_d_cs': (0.0051, 0.0037, 0.00047),
    '2176x2048x1024-drop_res': (0.0055, None, None),
    '2176x2048x1024-drop_gelu': (0.0051, 0.0056, None),
    '2176x2048x1024-drop_gelu_d': (0.0051, 0.0037, None),
    '2176x2048x1024-drop_res_cs': (0.0055, None, 0.00055),
    '2139x2048x256-bias': (0.022, None, None),
    '2139x2048x256-res': (0.023, None, None),
    '2139x2048x256-gelu_pre': (0.021, 0.022, None),
    '2139x2048x256-gelu_res': (0.021, None, None),
    '2139x2048x256-gelu_d': (0.021, 0.017, None),
    '2139x2048x256-gelu_bwd': (0.026, None, None),
    '2139x2048x256-mul': (0.026, None, None),
    '2139x2048x256-res_cs': (0.023, None, 0.0018),
    '2139x2048x256-gelu_d_cs': (0.021, 0.017, 0.0014),
    '2139x2048x256-drop_res': (0.024, None, None),
    '2139x2048x256-drop_gelu': (0.021, 0.022, None),
    '2139x2048x256-drop_gelu_d': (0.021, 0.017, None),
    '2139x2048x256-drop_res_cs': (0.024, None, 0.0015),
    '9856x640x256-bias': (0.025, None, None),
    '9856x640x256-res': (0.024, None, None),
    '9856x640x256-gelu_pre': (0.024, 0.025, None),
    '9856x640x256-gelu_res': (0.024, None, None),
    '9856x640x256-gelu_d': (0.024, 0.021, None),
    '9856x640x256-gelu_bwd': (0.025, None, None),
    '9856x640x256-mul': (0.027, None, None),
    '9856x640x256-res_cs': (0.024, None, 0.00078),
    '9856x640x256-gelu_d_cs': (0.024, 0.021, 0.00072),
    '9856x640x256-drop_res': (0.025, None, None),
    '9856x640x256-drop_gelu': (0.024, 0.025, None),
    '9856x640x256-drop_gelu_d': (0.024, 0.02, None),
    '9856x640x256-drop_res_cs': (0.025, None, 0.00074),
    '2176x2048x224-bias': (0.03, None, None),
    '2176x2048x224-res': (0.031, None, None),
    '2176x2048x224-gelu_pre': (0.026, 0.03, None),
    '2176x2048x224-gelu_res': (0.027, None, None),
    '2176x2048x224-gelu_d': (0.026, 0.021, None),
    '2176x2048x224-gelu_bwd': (0.035, None, None),
    '2176x2048x224-mul': (0.035, None, None),
    '2176x2048x224-res_cs': (0.031, None, 0.0017),
    '2176x2048x224-gelu_d_cs': (0.026, 0.021, 0.0015),
    '2176x2048x224-drop_res': (0.029, None, None),
    '2176x2048x224-drop_gelu': (0.028, 0.03, None),
    '2176x2048x224-drop_gelu_d': (0.027, 0.02, None),
    '2176x2048x224-drop_res_cs': (0.029, None, 0.002),
    '5x2x32-gelu_pre': (0.018, 0.016, None),
    '5x2x32-gelu_d': (0.018, 0.0026, None),
    '5x2x32-gelu_bwd': (0.012, None, None),
    '5x2x32-mul': (0.037, None, None),
    '5x2x48-gelu_pre': (0.01, 0.012, None),
    '5x2x48-gelu_d': (0.01, 0.0033, None),
    '5x2x48-gelu_bwd': (0.012, None, None),
    '5x2x48-mul': (0.013, None, None),
    '5x130x32-gelu_pre': (0.049, 0.088, None),
    '5x130x32-gelu_d': (0.049, 0.034, None),
    '5x130x32-gelu_bwd': (0.069, None, None),
    '5x130x32-mul': (0.099, None, None),
    '5x128x48-gelu_pre': (0.043, 0.04, None),
    '5x128x48-gelu_d': (0.043, 0.036, None),
    '5x128x48-gelu_bwd': (0.046, None, None),
    '5x128x48-mul': (0.067, None, None),
    '5x128x48-res_cs': (0.059, None, 0.021),
    '5x128x48-gelu_d_cs': (0.043, 0.036, 0.021),
    '5x130x48-gelu_pre': (0.046, 0.046, None),
    '5x130x48-gelu_d': (0.046, 0.019, None),
    '5x130x48-gelu_bwd': (0.042, None, None),
    '5x130x48-mul': (0.051, None, None),
    '128x130x32-bias': (0.16, None, None),
    '128x130x32-res': (0.16, None, None),
    '128x130x32-gelu_pre': (0.093, 0.16, None),
    '128x130x32-gelu_res': (0.075, None, None),
    '128x130x32-gelu_d': (0.093, 0.059, None),
    '128x130x32-gelu_bwd': (0.11, None, None),
    '128x130x32-mul': (0.18, None, None),
    '128x128x48-bias': (0.076, None, None),
    '128x128x48-res': (0.071, None, None),
    '128x128x48-gelu_pre': (0.064, 0.076, None),
    '128x128x48-gelu_res': (0.057, None, None),
    '128x128x48-gelu_d': (0.064, 0.049, None),
    '128x128x48-gelu_bwd': (0.076, None, None),
    '128x128x48-mul': (0.094, None, None),
    '128x128x48-res_cs': (0.071, None, 0.014),
    '128x128x48-gelu_d_cs': (0.064, 0.049, 0.018),
    '129x128x48-bias': (0.065, None, None),
    '129x128x48-res': (0.064, None, None),
    '129x128x48-gelu_pre': (0.052, 0.065, None),
    '129x128x48-gelu_res': (0.053, None, None),
    '129x128x48-gelu_d': (0.052, 0.041, None),
    '129x128x48-gelu_bwd': (0.08, None, None),
    '129x128x48-mul': (0.088, None, None),
    '129x128x48-res_cs': (0.064, None, 0.013),
    '129x128x48-gelu_d_cs': (0.052, 0.041, 0.012),
    '128x130x48-bias': (0.063, None, None),
    '128x130x48-res': (0.067, None, None),
    '128x130x48-gelu_pre': (0.057, 0.063, None),
    '128x130x48-gelu_res': (0.057, None, None),
    '128x130x48-gelu_d': (0.057, 0.046, None),
    '128x130x48-gelu_bwd': (0.063, None, None),
    '128x130x48-mul': (0.11, None, None),
    '129x130x48-bias': (0.072, None, None),
    '129x130x48-res': (0.073, None, None),
    '129x130x48-gelu_pre': (0.053, 0.072, None),
    '129x130x48-gelu_res': (0.056, None, None),
    '129x130x48-gelu_d': (0.053, 0.049, None),
    '129x130x48-gelu_bwd': (0.072, None, None),
    '129x130x48-mul': (0.088, None, None),
    '6619x640x256-bias': (0.028, None, None),
    '6619x640x256-res': (0.028, None, None),
    '6619x640x256-gelu_pre': (0.028, 0.028, None),
    '6619x640x256-gelu_res': (0.028, None, None),
    '6619x640x256-gelu_d': (0.028, 0.018, None),
    '6619x640x256-gelu_bwd': (0.026, None, None),
    '6619x640x256-mul': (0.031, None, None),
    '6619x640x256-res_cs': (0.028, None, 0.00088),
    '6619x640x256-gelu_d_cs': (0.028, 0.018, 0.00095),
    '6619x640x256-drop_res': (0.028, None, None),
    '6619x640x256-drop_gelu': (0.028, 0.028, None),
    '6619x640x256-drop_gelu_d': (0.028, 0.018, None),
    '6619x640x256-drop_res_cs': (0.028, None, 0.00082),
    '6619x640x384-bias': (0.017, None, None),
    '6619x640x384-res': (0.017, None, None),
    '6619x640x384-gelu_pre': (0.014, 0.017, None),
    '6619x640x384-gelu_res': (0.014, None, None),
    '6619x640x384-gelu_d': (0.014, 0.012, None),
    '6619x640x384-gelu_bwd': (0.017, None, None),
    '6619x640x384-mul': (0.018, None, None),
    '6619x640x384-res_cs': (0.017, None, 0.00077),
    '6619x640x384-gelu_d_cs': (0.014, 0.012, 0.00069),
    '6619x640x384-drop_res': (0.017, None, None),
    '6619x640x384-drop_gelu': (0.014, 0.017, None),
    '6619x640x384-drop_gelu_d': (0.014, 0.012, None),
    '6619x640x384-drop_res_cs': (0.017, None, 0.00083),
    '2139x2048x384-bias': (0.017, None, None),
    '2139x2048x384-res': (0.017, None, None),
    '2139x2048x384-gelu_pre': (0.016, 0.017, None),
    '2139x2048x384-gelu_res': (0.017, None, None),
    '2139x2048x384-gelu_d': (0.016, 0.013, None),
    '2139x2048x384-gelu_bwd': (0.018, None, None),
    '2139x2048x384-mul': (0.018, None, None),
    '2139x2048x384-res_cs': (0.017, None, 0.0016),
    '2139x2048x384-gelu_d_cs': (0.016, 0.013, 0.0012),
    '2139x2048x384-drop_res': (0.017, None, None),
    '2139x2048x384-drop_gelu': (0.016, 0.017, None),
    '2139x2048x384-drop_gelu_d': (0.016, 0.013, None),
    '2139x2048x384-drop_res_cs': (0.017, None, 0.0013),
    '6619x640x1024-bias': (0.0048, None, None),
    '6619x640x1024-res': (0.0049, None, None),
    '6619x640x1024-gelu_pre': (0.0035, 0.0048, None),
    '6619x640x1024-gelu_res': (0.0035, None, None),
    '6619x640x1024-gelu_d': (0.0035, 0.0037, None),
    '6619x640x1024-gelu_bwd': (0.0051, None, None),
    '6619x640x1024-mul': (0.0057, None, None),
    '6619x640x1024-res_cs': (0.0049, None, 0.00056),
    '6619x640x1024-gelu_d_cs': (0.0035, 0.0037, 0.0005),
    '6619x640x1024-drop_res': (0.0048, None, None),
    '6619x640x1024-drop_gelu': (0.0034, 0.0048, None),
    '6619x640x1024-drop_gelu_d': (0.0034, 0.0037, None),
    '6619x640x1024-drop_res_cs': (0.0048, None, 0.00053),
    '2139x2048x1024-bias': (0.0043, None, None),
    '2139x2048x1024-res': (0.0044, None, None),
    '2139x2048x1024-gelu_pre': (0.0036, 0.0043, None),
    '2139x2048x1024-gelu_res': (0.0035, None, None),
    '2139x2048x1024-gelu_d': (0.0036, 0.0039, None),
    '2139x2048x1024-gelu_bwd': (0.0047, None, None),
    '2139x2048x1024-mul': (0.0049, None, None),
    '2139x2048x1024-res_cs': (0.0044, None, 0.00062),
    '2139x2048x1024-gelu_d_cs': (0.0036, 0.0039, 0.00052),
    '2139x2048x1024-drop_res': (0.0042, None, None),
    '2139x2048x1024-drop_gelu': (0.0036, 0.0043, None),
    '2139x2048x1024-drop_gelu_d': (0.0036, 0.0039, None),
    '2139x2048x1024-drop_res_cs': (0.0042, None, 0.00058),
}
# case id -> written figure
TN_FP32_ERR = {
    'M1-128x128': 0.6,
    'M31-130x36': 0.11,
    'M32-36x260': 0.11,
    'M33-260x130': 0.13,
    'M64-128x128': 0.073,
    'M65-130x36': 0.055,
    'M97-36x260': 0.037,
    'M160-260x130': 0.03,
    'M511-128x128': 0.0056,
    'M4321-128x128': 0.00015,
    'M512-130x36': 0.0046,
    'M513-36x260': 0.0046,
    'M2049-128x128': 0.00058,
    'M4321-128x128-wgs16': 0.00015,
    'M16385-256x256': 2.9e-05,
    'M800-260x130-wgs12': 0.0033,
    'M1-36x260': 0.6,
    'M1-260x130': 0.6,
    'M32-130x36': 0.13,
    'M33-130x36': 0.15,
    'M64-130x36': 0.055,
    'M33-36x260': 0.15,
    'M96-130x36': 0.037,
    'M97-130x36': 0.036,
    'M32-128x128': 0.12,
    'M33-128x128': 0.12,
    'M64-36x260': 0.055,
    'M128-130x36': 0.029,
    'M65-36x260': 0.07,
    'M160-130x36': 0.024,
    'M96-36x260': 0.045,
    'M65-128x128': 0.058,
    'M32-260x130': 0.14,
    'M128-36x260': 0.032,
    'M257-130x36': 0.015,
    'M160-36x260': 0.031,
    'M96-128x128': 0.041,
    'M97-128x128': 0.072,
    'M128-128x128': 0.038,
    'M64-260x130': 0.07,
    'M65-260x130': 0.073,
    'M511-130x36': 0.0039,
    'M513-130x36': 0.005,
    'M257-36x260': 0.017,
    'M544-130x36': 0.0049,
    'M545-130x36': 0.0043,
    'M160-128x128': 0.03,
    'M577-130x36': 0.004,
    'M608-130x36': 0.0044,
    'M96-260x130': 0.048,
    'M97-260x130': 0.047,
    'M800-130x36': 0.0035,
    'M257-128x128': 0.019,
    'M128-260x130': 0.038,
    'M511-36x260': 0.0049,
    'M512-36x260': 0.0063,
    'M544-36x260': 0.0056,
    'M545-36x260': 0.0062,
    'M577-36x260': 0.0046,
    'M608-36x260': 0.0049,
    'M800-36x260': 0.0023,
    'M512-128x128': 0.0054,
    'M513-128x128': 0.0058,
    'M257-260x130': 0.024,
    'M544-128x128': 0.0061,
    'M545-128x128': 0.006,
    'M577-128x128': 0.0047,
    'M2049-130x36': 0.00053,
    'M608-128x128': 0.0053,
    'M800-128x128': 0.0025,
    'M511-260x130': 0.006,
    'M512-260x130': 0.0046,
    'M513-260x130': 0.006,
    'M545-260x130': 0.0054,
    'M2049-36x260': 0.00053,
    'M577-260x130': 0.0048,
    'M608-260x130': 0.0063,
    'M800-260x130': 0.0033,
    'M2049-260x130': 0.00059,
}
BATCHED_FP32_ERR = {
    '70x37x131-b1h1-kk': 0.028,
    '70x37x131-b1h1-kT': 0.028,
    '70x37x131-b1h1-Tk': 0.028,
    '70x37x131-b1h1-TT': 0.028,
    '37x64x131-b2h3-kk': 0.031,
    '37x64x131-b2h3-kT': 0.031,
    '37x64x131-b2h3-Tk': 0.031,
    '37x64x131-b2h3-TT': 0.031,
    '70x37x2051-b1h1-kk': 0.002,
    '70x37x2051-b1h1-kT': 0.002,
    '70x37x2051-b1h1-Tk': 0.002,
    '70x37x2051-b1h1-TT': 0.002,
    '37x64x2051-b2h3-kk': 0.0019,
    '37x64x2051-b2h3-kT': 0.0019,
    '37x64x2051-b2h3-Tk': 0.0019,
    '37x64x2051-b2h3-TT': 0.0019,
}
QUANTITIES = ('out', 'pre', 'colsum')


def lin_figures(key):
    return {q: f for q, f in zip(QUANTITIES, LIN_FP32_ERR[key]) if f is not None}


def lin_exact(e, q):
    """Integer flavour: is quantity q of epilogue e free of transcendentals (hence exact)?"""
    if q == 'pre':
        return e.act != P.ACT_GELU_D
    return e.act in (P.ACT_NONE, P.ACT_MUL)


class Knobs:
    """Tuning knobs for the length of a `with`: set on entry, back to 0 (the default) on exit."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        from valle2_amd import _lib
        try:
            for k, v in self.kv.items():
                assert _lib.lib().vh_set_tuning(int(k[1:]), v) == 0
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        from valle2_amd import _lib
        for k in self.kv:
            _lib.lib().vh_set_tuning(int(k[1:]), 0)


def framed(rows, cols, fill=SENT, extra_rows=2):
    """A (rows, cols) view with row stride pad4(cols) + 4 inside a larger buffer full of `fill`; returns (buffer, view)."""
    buf = torch.full((rows + extra_rows, P.pad4(cols) + 4), fill, device=DEV)
    return buf, buf[:rows, :cols]


def frame_kept(buf, rows, cols, fill=SENT):
    return bool((buf[rows:] == fill).all()) and bool((buf[:, cols:] == fill).all())


def padded_operand(t, pad_to=None):
    """Device copy of a 2-D operand whose rows are followed by NaN (beyond `pad_to` columns, which hold what t holds)."""
    r, c = t.shape
    buf = torch.full((r, P.pad4(c) + 4), float('nan'))
    buf[:, :c] = t
    return buf.to(DEV)[:, :c if pad_to is None else pad_to]


def close(got, ref, cap, factor):
    """max |got - ref| / (factor x cap) on the device, in float64; <= 1 passes."""
    return P.worst_ratio(got, ref, cap * factor)


# ======================================================================================================================
# vh_linear_ex
# ======================================================================================================================
class LinRun:
    """The device side of one (geometry, flavour): operands with NaN padding, launched through the ctypes entry."""

    def __init__(self, g, flavour):
        from valle2_amd import dropout
        self.g, self.flavour = g, flavour
        inp = P.lin_inputs(g, flavour)
        self.a = padded_operand(inp['a'])
        self.w = inp['w'].to(DEV)
        self.bias = inp['bias'].to(DEV)
        self.res = {k: padded_operand(inp[k]) for k in ('res', 'saved')}
        self.spec = dropout.spec(P.DROP_SEED, P.DROP_SITE, P.DROP_P[flavour])

    def launch(self, e, ws_bytes):
        """One launch with a NaN workspace of ws_bytes bytes -> {quantity: device tensor}; the sentinel frames are checked."""
        from valle2_amd import _lib, kernels as K
        g = self.g
        obuf, out = framed(g.M, g.N)
        pbuf, pre = framed(g.M, g.N) if e.pre_out else (None, None)
        cs = None
        if e.colsum:
            cs = torch.full((g.N + 4,), SENT, device=DEV)
            cs[:g.N] = 0.0
        ws = torch.full(((ws_bytes + 3) // 4,), float('nan'), device=DEV) if ws_bytes else None
        r = None if e.res is None else self.res['res' if e.res == 'res' else 'saved']
        K.check(_lib.lib().vh_linear_ex(
            self.a.data_ptr(), self.a.stride(0), self.w.data_ptr(), self.bias.data_ptr() if e.bias else None,
            r.data_ptr() if r is not None else None, r.stride(0) if r is not None else 0, out.data_ptr(), out.stride(0),
            pre.data_ptr() if pre is not None else None, pre.stride(0) if pre is not None else 0,
            cs.data_ptr() if cs is not None else None, g.M, g.N, g.K, e.act, C.byref(self.spec) if e.drop else None,
            ws.data_ptr() if ws is not None else None, ws_bytes, K.stream()), 'vh_linear_ex')
        got = {'out': out}
        assert frame_kept(obuf, g.M, g.N), 'out: rows >= M / columns >= N were written'
        if pre is not None:
            got['pre'] = pre
            assert frame_kept(pbuf, g.M, g.N), 'pre_out: rows >= M / columns >= N were written'
        if cs is not None:
            got['colsum'] = cs[:g.N]
            assert bool((cs[g.N:] == SENT).all()), 'colsum: columns >= N were written'
        return got


def lin_keys():
    seen = []
    for c in P.lin_cases():
        if P.lin_figure_key(c) not in seen:
            seen.append(P.lin_figure_key(c))
    return seen


@pytest.fixture(scope='module')
def lin_run():
    """(geometry, flavour) -> its LinRun; the last geometry's two are kept (the cases come geometry by geometry) and let go
    with the module."""
    runs = {}

    def get(g, flavour):
        if (g, flavour) not in runs:
            if len(runs) >= 2:
                runs.clear()
            runs[(g, flavour)] = LinRun(g, flavour)
        return runs[(g, flavour)]
    yield get
    runs.clear()


@pytest.mark.parametrize('key', lin_keys())
def test_linear_ex_case(key, lin_run):
    """One (geometry, epilogue) on every staging that accepts it, both flavours, with and without the tail split."""
    from valle2_amd import _lib
    cases = [c for c in P.lin_cases() if P.lin_figure_key(c) == key]
    g, e = cases[0].geom, P.epi_of(cases[0].epi)
    need = _lib.lib().vh_linear_ex_ws_bytes(g.M, g.N, g.K)
    assert need == P.linear_ex_ws_bytes(g.M, g.N, g.K)
    for flavour in ('float', 'int'):
        run = lin_run(g, flavour)
        ref = {q: (v.to(DEV), cap.to(DEV)) for q, (v, cap) in P.lin_reference(cases[0], flavour).items()}
        figs = lin_figures(key)

        def check(got, what):
            for q, (v, cap) in ref.items():
                if flavour == 'int' and lin_exact(e, q):
                    assert torch.equal(got[q].double(), v), f'{what} {q}: integer operands must come out exactly'
                else:
                    factor = P.bound_factor(figs[q]) if flavour == 'float' else 1.0
                    miss = close(got[q], v, cap, factor)
                    print(f'{key} {what} {flavour} {q}: {miss:.3f} of the bound ({factor:.3g} x cap)')
                    assert miss <= 1.0, f'{what} {q}: {miss:.2f} x the bound'

        for c in cases:
            sig = P.lin_signature(*g, tile_dma=c.tile_dma)
            with Knobs(k4=c.tile_dma):
                got = run.launch(e, need)
                again = run.launch(e, need)
                check(got, f'dma{c.tile_dma}')
                for q in got:
                    if q != 'colsum':
                        assert torch.equal(got[q], again[q]), f'{q}: a second launch differs'
                if not sig.split:
                    continue
                with Knobs(k10=1):
                    unsplit = run.launch(e, need)
                short = run.launch(e, need - 1)              # a workspace one byte short: the unsplit launch (launch_form)
                check(unsplit, 'unsplit')
                tail = P.tail_mask(g, P.tail_plan(*g)[1]).to(DEV)
                for q in got:
                    if q == 'colsum':
                        continue
                    assert torch.equal(short[q], unsplit[q]), f'{q}: a short workspace must give the unsplit launch'
                    assert torch.equal(got[q][~tail], unsplit[q][~tail]), f'{q}: whole tiles differ between split and unsplit'
                    if not (flavour == 'int' and lin_exact(e, q)):
                        v, cap = ref[q]
                        factor = P.bound_factor(figs[q]) if flavour == 'float' else 1.0
                        apart = close(got[q], unsplit[q].double(), cap, factor)
                        print(f'{key} split against unsplit {flavour} {q}: {apart:.3f} of the bound')
                        assert apart <= 1.0, f'{q}: tail tiles, split against unsplit: {apart:.2f} x the bound'


def test_dropout_field_of_the_cases_is_the_oracles():
    from valle2_amd import dropout
    for flavour in ('float', 'int'):
        sp = dropout.spec(P.DROP_SEED, P.DROP_SITE, P.DROP_P[flavour])
        keep = dropout.mask(sp, 130, 256, DEV).cpu().float()
        assert torch.equal(keep, P.keep_field(flavour, 130, 256))


# ======================================================================================================================
# vh_gemm_tn
# ======================================================================================================================
def tn_launch(c, a, b, ws_bytes):
    """(return code, C view, C buffer) of one vh_gemm_tn launch with a NaN workspace of ws_bytes bytes."""
    from valle2_amd import _lib, kernels as K
    cbuf, out = framed(c.NI, c.NJ)
    ws = torch.full(((ws_bytes + 3) // 4,), float('nan'), device=DEV) if ws_bytes > 0 else None
    rc = _lib.lib().vh_gemm_tn(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0), c.M, c.NI, c.NJ,
                               ws.data_ptr() if ws is not None else None, max(ws_bytes, 0), K.stream())
    torch.cuda.synchronize()
    return rc, out, cbuf


@pytest.mark.parametrize('c', P.tn_cases(), ids=P.tn_case_id)
def test_gemm_tn_case(c):
    from valle2_amd import _lib
    with Knobs(k11=c.wgs):
        need = _lib.lib().vh_gemm_tn_ws_bytes(c.M, c.NI, c.NJ)
        assert need == P.tn_ws_bytes(*c)
        for flavour in ('float', 'int'):
            a, b = P.tn_inputs(c, flavour)
            ad, bd = a.to(DEV)[:, :c.NI], b.to(DEV)[:, :c.NJ]
            rc, out, cbuf = tn_launch(c, ad, bd, need)
            assert rc == 0 and frame_kept(cbuf, c.NI, c.NJ), 'vh_gemm_tn wrote outside C'
            ref, S = P.tn_reference(c, flavour)
            if flavour == 'int':
                assert torch.equal(out.cpu().double(), ref), 'integer operands must come out exactly'
            else:
                miss = close(out.cpu(), ref, P.tn_cap(c, S), P.bound_factor(TN_FP32_ERR[P.tn_case_id(c)]))
                print(f'{P.tn_case_id(c)}: {miss:.3f} of the bound')
                assert miss <= 1.0
            rc2, out2, _ = tn_launch(c, ad, bd, need)
            assert rc2 == 0 and torch.equal(out, out2), 'slab sums must be bitwise reproducible'
        if need:
            rc, _, _ = tn_launch(c, ad, bd, need - 1)
            assert rc != 0, 'a workspace one byte short must be refused'


# ======================================================================================================================
# transposes
# ======================================================================================================================
@pytest.mark.parametrize('rows,cols,ldo', P.TRANSPOSE_CASES)
def test_transpose_case(rows, cols, ldo):
    from valle2_amd import kernels as K
    w = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows * 1000 + cols))
    buf = torch.full((cols + 2, ldo), SENT, device=DEV)
    wd = padded_operand(w)
    K.transpose(wd, ldo=ldo, out=buf[:cols])
    assert torch.equal(buf[:cols].cpu(), P.transpose_emulate(w, ldo)) and bool((buf[cols:] == SENT).all())
    again = torch.full((cols, ldo), SENT, device=DEV)
    assert torch.equal(K.transpose(wd, ldo=ldo, out=again), buf[:cols])


@pytest.mark.parametrize('n', P.PLAN_COUNTS)
def test_transpose_plan(n):
    """vh_transpose_many over n items (its item search strides by 64): every output is w^T with zero padding, before and after
    an in-place update of the weights."""
    from valle2_amd import kernels as K
    weights, ldos = P.plan_weights(n)
    wd = [padded_operand(w) for w in weights]
    plan = K.TransposePlan(wd, ldos)
    assert plan.tiles == sum(P.cdiv(w.shape[1], 32) * P.cdiv(ldo, 32) for w, ldo in zip(weights, ldos))
    for rnd in range(2):
        for o in plan.outs:
            o.fill_(SENT)
        outs = plan.run()
        first = [o.clone() for o in outs]
        for i, (w, ldo, o) in enumerate(zip(wd, ldos, outs)):
            want = torch.zeros(w.shape[1], ldo)
            want[:, :w.shape[0]] = w.cpu().T
            assert torch.equal(o.cpu(), want), f'item {i} of {n} {tuple(w.shape)} ldo {ldo}, round {rnd}'
        assert all(torch.equal(x, y) for x, y in zip(first, plan.run()))
        for i, w in enumerate(wd):                              # the optimizer's in-place step
            w.mul_(-0.5).add_(float(i + 1))


# ======================================================================================================================
# vh_gemm_batched
# ======================================================================================================================
def batched_view(t, kmajor):
    """(nb, nh, rows, cols) -> a device view read in place: 2-D when nb = nh = 1, else strided over a (nb, rows, nh, ld) buffer;
    k-major operands are stored transposed.  The row stride is pad4(cols) + 4 with NaN beyond the pad."""
    if kmajor:
        t = t.transpose(-1, -2)
    nb, nh, rows, cols = t.shape
    ld = P.pad4(cols) + 4
    gen = torch.Generator().manual_seed(rows * cols)
    buf = torch.randn(nb, rows, nh, ld, generator=gen)          # the pad holds finite values nobody may use
    buf[..., P.pad4(cols):] = float('nan')
    buf[..., :cols] = t.permute(0, 2, 1, 3)
    v = buf.to(DEV).permute(0, 2, 1, 3)[..., :cols]
    return v[0, 0] if nb == nh == 1 else v


@pytest.mark.parametrize('c', P.batched_cases(), ids=P.batched_case_id)
def test_gemm_batched_case(c):
    from valle2_amd import kernels as K
    split = P.batched_splits(c.M, c.N, c.K, c.nb, c.nh)
    assert (split > 1) == (c.K >= 2048)
    for flavour in ('float', 'int'):
        a, b = P.batched_inputs(c, flavour)
        ref, S = P.batched_reference(c, flavour)
        obuf = torch.full((c.nb, c.M + 1, c.nh, P.pad4(c.N) + 4), SENT, device=DEV)
        out = obuf.permute(0, 2, 1, 3)[:, :, :c.M, :c.N]
        av, bv = batched_view(a, c.ak), batched_view(b, c.bk)
        K.gemm(av, bv, out[0, 0] if c.nb == c.nh == 1 else out, a_kmajor=c.ak, b_kmajor=c.bk)
        if split == 1:                                          # no atomics: a second launch gives the same bits
            again = torch.empty_like(obuf).permute(0, 2, 1, 3)[:, :, :c.M, :c.N]
            K.gemm(av, bv, again[0, 0] if c.nb == c.nh == 1 else again, a_kmajor=c.ak, b_kmajor=c.bk)
            assert torch.equal(out, again), 'a second launch differs'
        assert bool((obuf[:, c.M:] == SENT).all()) and bool((obuf[..., c.N:] == SENT).all()), 'wrote outside the output'
        if flavour == 'int':
            assert torch.equal(out.cpu().double(), ref)
        else:
            miss = close(out.cpu(), ref, P.batched_cap(c, S), P.bound_factor(BATCHED_FP32_ERR[P.batched_case_id(c)]))
            print(f'{P.batched_case_id(c)}: {miss:.3f} of the bound')
            assert miss <= 1.0
