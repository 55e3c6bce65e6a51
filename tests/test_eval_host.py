"""Host side of the forward-only objective (rae_eval_cost, include/rae.h): the ctypes struct
layout, the argument check (which runs before any HIP call, so it works without a GPU), the
bounded workspace and the command line flags.  No GPU needed."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT


def test_eval_args_offsets_match_c_compiler(tmp_path):
    """Every rae_eval_args field sits at the offset the C compiler gives it (the method of
    test_abi.test_struct_offsets_match_c_compiler)."""
    from rae import _lib
    src = tmp_path / "off.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rae.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(rae_eval_args));']
    for fname, _ in _lib.RaeEvalArgs._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(rae_eval_args, {fname}));')
    lines.append("return 0; }")
    src.write_text("\n".join(lines))
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = dict(line.rsplit(" ", 1) for line in out.split("\n") if line)
    assert int(got["size"]) == C.sizeof(_lib.RaeEvalArgs)
    for fname, _ in _lib.RaeEvalArgs._fields_:
        assert int(got[fname]) == getattr(_lib.RaeEvalArgs, fname).offset, fname


def _args(decoder=0, m=100, r=200, s=20, nrows=1000):
    """Well-formed arguments with made-up (never dereferenced) aligned device addresses."""
    from rae import _lib
    a = _lib.RaeEvalArgs()
    a.decoder, a.relations, a.embed, a.neg_samples = decoder, m, r, s
    a.n_entities, a.alpha = 1000, 1.0
    fake = 0x10000
    for f in ("W", "Wb", "A", "Ab", "C1", "C2", "R3", "indptr", "indices", "args1", "args2",
              "neg1", "neg2", "sums_out", "workspace"):
        setattr(a, f, fake)
        fake += 0x10000
    a.neg_stride, a.row0, a.nrows = nrows, 0, nrows
    return a


def _ws(lib, a):
    return int(lib.rae_eval_workspace_bytes(C.byref(a)))


@pytest.mark.parametrize("decoder", [0, 1, 2])
def test_eval_cost_rejects_bad_arguments(built_lib, decoder):
    lib = built_lib
    bad = []

    def case(name, word, **change):
        a = _args(decoder)
        a.workspace_bytes = _ws(lib, a)
        assert a.workspace_bytes > 0
        for k, v in change.items():
            setattr(a, k, v)
        if "short" in name:
            a.workspace_bytes -= 1
        rc = lib.rae_eval_cost(C.byref(a), None)
        msg = lib.rae_last_error().decode()
        if rc != -1 or word not in msg:
            bad.append((name, rc, msg))

    case("null W", "W", W=None)
    case("decoder 7", "decoder", decoder=7)
    case("neg_samples 0", "neg_samples", neg_samples=0)
    case("nrows -1", "nrows", nrows=-1)
    case("short workspace", "workspace_bytes")
    case("null sums", "sums_out", sums_out=None)
    case("relations 0", "relations", relations=0)
    case("embed 0", "embed", embed=0)
    case("short negatives", "neg_stride", neg_stride=10)
    assert not bad, bad


def test_eval_workspace_is_bounded(built_lib):
    lib = built_lib
    for decoder, m, r, s in ((0, 100, 200, 20), (0, 300, 300, 50), (1, 100, 200, 20),
                             (2, 30, 60, 10), (1, 7, 13, 3)):
        a6, a7 = _args(decoder, m, r, s, 10 ** 6), _args(decoder, m, r, s, 10 ** 7)
        assert _ws(lib, a6) == _ws(lib, a7) > 0, (decoder, m, r, s)
    # a shape the kernels do not handle is refused, not mis-sized
    assert _ws(lib, _args(1, 400, 200, 20)) == -1
    assert b"relations" in lib.rae_last_error()


def test_eval_shape_limits_one_step_past(built_lib):
    """The shape limits include/rae.h states (relations <= 512, a multiple of 4 above 128, <= 320
    for the bilinear decoders; embed <= 1024; at most 160 KiB of LDS per 16-example tile): the
    last accepted shape gives a positive size, one step past it gives -1 and rae_last_error
    names the field."""
    lib = built_lib
    SP, RESCAL, HYBRID = 0, 1, 2
    # the hybrid's tile holds P (m rounded up to 4) and four vectors of r rounded up to 4:
    # 16 (mS + 4 r4) 4 bytes <= 160 KiB; at m = 4 the largest r is 636
    r_hyb = max(r for r in range(1, 1025) if 16 * (4 + 4 * ((r + 3) & ~3)) * 4 <= 160 * 1024)
    assert r_hyb == 636
    accepted = [(SP, 512, 200), (SP, 128, 200), (SP, 127, 200), (SP, 100, 1024), (SP, 512, 1024),
                (RESCAL, 320, 24), (HYBRID, 320, 24), (HYBRID, 4, r_hyb)]
    for dec, m, r in accepted:
        assert _ws(lib, _args(dec, m, r, 3)) > 0, (dec, m, r, lib.rae_last_error())
    refused = [(SP, 513, 200, "relations"), (SP, 129, 200, "relations"),
               (SP, 130, 200, "relations"), (SP, 100, 1025, "embed"),
               (RESCAL, 324, 24, "relations"), (HYBRID, 324, 24, "relations"),
               (SP, 512, 1028, "embed"), (HYBRID, 4, r_hyb + 1, "embed"), (HYBRID, 4, 640, "embed")]
    bad = []
    for dec, m, r, word in refused:
        a = _args(dec, m, r, 3)
        size = _ws(lib, a)
        msg = lib.rae_last_error().decode()
        a.workspace_bytes = 1 << 40
        rc = lib.rae_eval_cost(C.byref(a), None)        # refused before any HIP call
        if size != -1 or rc != -1 or word not in msg:
            bad.append((dec, m, r, size, rc, msg))
    assert not bad, bad


def test_cli_eval_cost_flag():
    from rae import cli
    base = ["data.npz", "--model-name", "m", "--decoder", "sp"]
    a = cli.get_command_args(base)
    assert a.eval_cost is False and a.eval_seed is None
    # the reference's defaults are unchanged (learning/OieInduction.py:464-480)
    assert (a.epochs, a.learning_rate, a.batch_size, a.embed_size, a.relations, a.neg_samples,
            a.l1, a.l2, a.optimizer, a.alpha, a.seed) == (100, 0.1, 50, 30, 3, 5, 0.0, 0.0,
                                                           "adagrad", 1.0, 2)
    b = cli.get_command_args(base + ["--eval-cost", "--eval-seed", "11"])
    assert b.eval_cost is True and b.eval_seed == 11
