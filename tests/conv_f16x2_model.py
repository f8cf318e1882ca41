"""ctypes binding of tests/cpp/conv_f16x2_model.cpp — the CPU restatement of Connect4ConvNet in the f16x2 arithmetic (TEST INFRASTRUCTURE
ONLY). load(build_dir) compiles the library with g++ into the caller's directory (a test's tmp_path_factory directory, as
tests/test_cpp_host.py builds its harness), with the oracle's flags (oracle/Makefile). Its search and self-play calls take the argument
layout of the oracle's orc_c4conv_* calls, so tests/oracle_lib.py's marshalling and tests/test_gpu_parity.py's comparison helpers apply
as they are."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.oracle_lib import Oracle, _p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "conv_f16x2_model.cpp")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-mavx2", "-pthread"]   # oracle/Makefile


class _Calls:
    """The model's exports under the names tests/oracle_lib.Oracle calls for net="conv"."""

    def __init__(self, lib):
        lib.cf16_selfplay.restype = C.c_double
        lib.cf16_num_params.restype = C.c_size_t
        self.orc_c4conv_eval = lib.cf16_eval
        self.orc_c4conv_num_params = lib.cf16_num_params
        self.orc_c4conv_mcts_search = lib.cf16_mcts_search
        self.orc_c4conv_selfplay = lib.cf16_selfplay


class ConvF16x2Model:
    def __init__(self, lib):
        self.lib = lib
        self._o = Oracle.__new__(Oracle)   # (its marshalling only: the calls below go to the model's exports)
        self._o.lib = _Calls(lib)

    def eval(self, blob, my_bb, op_bb, raw=False):
        return self._o.c4conv_eval(blob, my_bb, op_bb, mode=Oracle.ACC_F16X2, raw=raw)

    def plan(self, blob):
        """None, or the plan as syn_f16x2_plan_of_blob reports it for a 12,412-float blob (layer 0 = conv, layer 1 = head)."""
        blob = np.ascontiguousarray(blob, np.float32)
        e = (C.c_int * 4)()
        b = (C.c_double * 2)()
        if not self.lib.cf16_plan(_p(blob), e, b):
            return None
        return dict(activation_exp=[0, e[1], 0, 0, 0], weight_exp=[e[0], e[2], 0, 0, 0], out_exp=e[3], bound=[b[0], b[1], 0.0, 0.0, 0.0])

    def mcts_search(self, cfg, blob, my_bb, op_bb, explores, action_selection=1):
        return self._o.c4_mcts_search(cfg, blob, my_bb, op_bb, explores, action_selection=action_selection, nn_mode=Oracle.ACC_F16X2,
                                      net="conv")

    def selfplay(self, cfg, blob, base_seed, n_games, first_game=0, threads=1, use_cache=False):
        return self._o.c4_selfplay(cfg, blob, base_seed, n_games, first_game=first_game, threads=threads, use_cache=use_cache,
                                   nn_mode=Oracle.ACC_F16X2, net="conv")


def load(build_dir):
    so = os.path.join(str(build_dir), "libconv_f16x2_model.so")
    subprocess.check_call(["g++"] + FLAGS + ["-shared", "-o", so, SRC])
    return ConvF16x2Model(C.CDLL(so))
