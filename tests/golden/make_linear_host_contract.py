"""Generate tests/golden/linear_host_contract.json: what the host side of the linear / convolution entry points answers.

    python tests/golden/make_linear_host_contract.py <path to a libcodetr_hip.so>

Run it on the library of the commit BEFORE a change to the launchers (build that commit in a scratch checkout), never on
the library under test: tests/test_linear_contract_cpu.py replays the table against the library it tests.

Two parts, both data:
  rows     [entry point, arguments, returned code]: calls that every launcher rejects on the host, before any HIP call
           (so they run without a GPU).  Every code is a negative CODETR_E_* value; the generator refuses a row the
           library accepts.  Pointer arguments are the integers 0 (null), 16 (never dereferenced) and 24 (misaligned);
           a list stands for a host array of int64 (the level shapes of the posgen entries, which ARE read).  An entry
           point written `stem_*` is stem_f16 and stem_bf16: both are called and must return the code.
  queries  codetr_linear_variant and codetr_linear_splitk_plan, pure functions of their arguments, over a grid of shapes
           (M x N x K) and every (act, residual, head dimension) of ACTS x (0, 1) x HEAD_DIMS, plus the shapes the GPU tests
           name.  Per (N, K): one letter per (M, act, residual, head dimension) and the plan per M.
"""
import ctypes
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "linear_host_contract.json")

NULL, P, BAD = 0, 16, 24
I31 = 0x7fffffff

GRID_M = [1, 127, 128, 300, 600, 900, 1444, 5000, 25599, 25600, 32767, 32768, 40000, 51200, 80640, 204600, 614400,
          614401, 818400]
GRID_N = [4, 64, 128, 192, 256, 1152, 1536, 1544, 4096]
GRID_K = [64, 192, 256, 320, 384, 1536, 2048, 6144, 13824]
# the shapes tests/test_linear_gpu.py names (M, N, K)
NAMED = [[204600, 256, 2048], [900, 256, 256], [1444, 768, 3072], [2048, 1024, 4096], [2176, 1024, 4096], [300, 64, 2048]]
ACTS, HEAD_DIMS = (0, 3), (0, 32, 64)
LETTER = {"tile128": "a", "tile256": "b", "xs": "x", "unsupported": "u"}


def bind(lib_path):
    """the library at lib_path with the signatures of include/codetr_hip.h, read as codetr/_cabi.py reads them (the reader
    is loaded by path: importing the package would load the product library beside it)"""
    spec = importlib.util.spec_from_file_location("_cheader", os.path.join(ROOT, "co-detr-tensorrt_amd", "codetr", "_cheader.py"))
    header = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(header)
    ctype = {"p": ctypes.c_void_p, "i": ctypes.c_int, "l": ctypes.c_int64, "f": ctypes.c_float, "s": ctypes.c_char_p}
    lib = ctypes.CDLL(lib_path)
    for name, (ret, params) in header.functions.items():
        if name.startswith(("codetr_linear", "codetr_conv_tokens", "codetr_encoder_projections")):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = ctype[header.kind(ret, returned=True)], [ctype[header.kind(t)] for t, _ in params]
    return lib


def entries(entry):
    """a row's entry points: `stem_*` stands for stem_f16 and stem_bf16, which must answer alike"""
    return [entry[:-1] + t for t in ("f16", "bf16")] if entry.endswith("_*") else [entry]


def call(lib, name, args):
    """one row: a list argument becomes an int64 array (kept alive for the call), everything else goes as it is"""
    keep = [(ctypes.c_int64 * len(a))(*a) if isinstance(a, list) else None for a in args]
    real = [ctypes.cast(k, ctypes.c_void_p) if k is not None else a for a, k in zip(args, keep)]
    return getattr(lib, name)(*real)


def variant_letters(lib, N, K, shapes_m):
    return "".join(LETTER[lib.codetr_linear_variant(M, N, K, act, res, hd).decode()]
                   for M in shapes_m for act in ACTS for res in (0, 1) for hd in HEAD_DIMS)


def plan(lib, M, N, K):
    ws = ctypes.c_int64(-1)
    splits = lib.codetr_linear_splitk_plan(M, N, K, ctypes.cast(ctypes.pointer(ws), ctypes.c_void_p))
    return [splits, ws.value]


def queries(lib):
    grid = {f"{N},{K}": {"variant": variant_letters(lib, N, K, GRID_M), "plan": [plan(lib, M, N, K) for M in GRID_M]}
            for N in GRID_N for K in GRID_K}
    named = [[M, N, K, variant_letters(lib, N, K, [M]), plan(lib, M, N, K)] for M, N, K in NAMED]
    return {"M": GRID_M, "acts": list(ACTS), "head_dims": list(HEAD_DIMS), "letters": LETTER, "grid": grid, "named": named}


def _vary(base, **changes):
    d = dict(base)
    d.update(changes)
    return d


def _cases(base, singles, combos=()):
    """base with one argument changed per case (singles: name -> values), then the cases that change several"""
    out = [_vary(base, **{k: v}) for k, vs in singles.items() for v in vs]
    return out + [_vary(base, **c) for c in combos]


def linear_rows():
    order = ("stream", "x", "w", "bias", "res", "mask", "y", "M", "N", "K", "act", "hm_rows", "hm_hd")
    base = dict(stream=NULL, x=P, w=P, bias=NULL, res=NULL, mask=NULL, y=P, M=1000, N=256, K=256, act=0, hm_rows=0, hm_hd=0)
    cases = _cases(base, {
        "x": [NULL, BAD], "w": [NULL, BAD], "y": [NULL],
        "M": [0, -1, I31 + 1], "N": [0, -5, I31 + 1], "K": [0, -64, 100, 2 ** 31],
        "act": [-1, 4],
    }, [
        dict(M=I31, N=I31),                       # the tile count of the 128-tile kernel
        dict(hm_hd=32), dict(hm_rows=100),        # one of the pair only
        dict(hm_hd=-8, hm_rows=100), dict(hm_hd=12, hm_rows=100), dict(hm_hd=48, hm_rows=100),
        dict(hm_hd=32, hm_rows=300), dict(hm_hd=32, hm_rows=-100), dict(hm_hd=32, hm_rows=100, res=P),
        dict(x=NULL, K=100), dict(K=100, M=I31 + 1), dict(act=4, M=I31 + 1), dict(x=BAD, M=I31 + 1),
        dict(x=BAD, hm_hd=12, hm_rows=100),       # the order of the checks
    ])
    return [["codetr_linear_*", [c[k] for k in order]] for c in cases]


def xs_domain():
    """outside the X-stationary kernel's domain, one bound each (K, N range, N % 8, M < 32768)"""
    return [dict(K=384), dict(K=64), dict(K=320), dict(N=120), dict(N=1544), dict(N=260), dict(M=32767)]


def f16out_rows():
    order = ("stream", "x", "w", "bias", "mask", "y", "M", "N", "K", "hm_rows", "hm_hd")
    base = dict(stream=NULL, x=P, w=P, bias=NULL, mask=NULL, y=P, M=40000, N=256, K=256, hm_rows=0, hm_hd=0)
    cases = _cases(base, {
        "x": [NULL, BAD], "w": [NULL, BAD], "y": [NULL, BAD], "M": [0, -1, I31 + 1], "N": [0, I31 + 1], "K": [0, -256],
    }, xs_domain() + [
        dict(hm_hd=32), dict(hm_rows=100), dict(hm_hd=-8, hm_rows=100), dict(hm_hd=12, hm_rows=100),
        dict(hm_hd=48, hm_rows=100), dict(hm_hd=32, hm_rows=300), dict(hm_hd=32, hm_rows=-100),
        dict(x=BAD, M=I31 + 1), dict(x=BAD, K=384), dict(hm_hd=12, hm_rows=100, y=BAD),
    ])
    return [["codetr_linear_bf16_f16out", [c[k] for k in order]] for c in cases]


def xadd_rows():
    order = ("stream", "x", "x2", "w", "bias", "y", "M", "N", "K")
    base = dict(stream=NULL, x=P, x2=P, w=P, bias=NULL, y=P, M=40000, N=256, K=256)
    cases = _cases(base, {
        "x": [NULL, BAD], "x2": [NULL, BAD], "w": [NULL, BAD], "y": [NULL, BAD],
        "M": [0, -1, I31 + 1], "N": [0, I31 + 1], "K": [0, -256],
    }, xs_domain() + [dict(x=NULL, M=I31 + 1), dict(y=BAD, M=I31 + 1)])
    return [["codetr_linear_xadd_*", [c[k] for k in order]] for c in cases]


def ln_rows():
    order = ("stream", "x", "g", "b", "eps", "w", "bias", "y", "M", "N", "K", "act")
    base = dict(stream=NULL, x=P, g=P, b=P, eps=1e-5, w=P, bias=NULL, y=P, M=40000, N=256, K=256, act=0)
    cases = _cases(base, {
        "x": [NULL, BAD], "g": [NULL, BAD], "b": [NULL, BAD], "w": [NULL, BAD], "y": [NULL, BAD],
        "M": [0, -1, I31 + 1], "N": [0, I31 + 1], "K": [0, -256], "act": [-1, 3, 4],
    }, xs_domain() + [dict(act=3, M=I31 + 1), dict(y=BAD, M=I31 + 1)])
    return [["codetr_linear_ln_*", [c[k] for k in order]] for c in cases]


def splitk_rows():
    order = ("stream", "x", "w", "bias", "res", "mask", "y", "M", "N", "K", "act", "splits", "ws", "ws_bytes")
    M, N = 600, 256
    base = dict(stream=NULL, x=P, w=P, bias=NULL, res=NULL, mask=NULL, y=P, M=M, N=N, K=13824, act=0, splits=4, ws=P,
                ws_bytes=1 << 60)
    cases = _cases(base, {
        "x": [NULL, BAD], "w": [NULL, BAD], "y": [NULL], "ws": [NULL, BAD],
        "M": [0, -1, I31 + 1], "N": [0, I31 + 1], "K": [0, -64, 100, 2 ** 31], "act": [-1, 3, 4],
        "splits": [1, 0, -2, 65536, 100],          # 100: 216 k-tiles in ranges of 3 leave the last ranges empty
        "ws_bytes": [4 * M * N * 4 - 1, 0],
    }, [dict(splits=1, K=100), dict(act=3, M=I31 + 1), dict(x=BAD, splits=65536), dict(x=BAD, ws_bytes=0),
        dict(splits=100, ws_bytes=0)])
    return [["codetr_linear_splitk_*", [c[k] for k in order]] for c in cases]


def conv_rows():
    order = ("stream", "x", "w", "bias", "res", "y", "B", "H", "W", "C", "Cout", "k", "stride", "pad", "act")
    base = dict(stream=NULL, x=P, w=P, bias=NULL, res=NULL, y=P, B=1, H=32, W=32, C=64, Cout=64, k=3, stride=1, pad=1, act=0)
    cases = _cases(base, {
        "x": [NULL, BAD], "w": [NULL, BAD], "y": [NULL, BAD], "res": [BAD], "bias": [BAD],
        "B": [0, -1, 2 ** 31], "H": [0, 0x10000], "W": [0, 0x10000], "C": [0, 96, 2 ** 28], "Cout": [0, 12, 2 ** 31],
        "k": [0, 2, 5], "stride": [0, 3], "pad": [-1, 3], "act": [-1, 4],
    }, [
        dict(k=1, pad=1),                                        # pad >= k
        dict(H=2, pad=0), dict(W=1, pad=0),                      # no output pixel
        dict(B=I31, H=1, W=1, k=1, pad=0, Cout=I31 - 7),         # the tile count
        dict(x=NULL, k=2), dict(k=2, x=BAD), dict(x=BAD, H=2, pad=0), dict(H=0x10000, W=1, pad=0, k=1),
    ])
    return [["codetr_conv_tokens_*", [c[k] for k in order]] for c in cases]


# what split_check tests, as changes to an accepted call of either SPLIT entry point (second: the operand of the second
# product that must be aligned -- the positional tensor, or the level embedding)
def split_cases(second):
    return _cases({}, {
        "x": [NULL, BAD], "w": [NULL, BAD], "value": [NULL, BAD], "packed": [NULL, BAD], "bias": [BAD], second: [BAD],
        "M": [0, -1, I31 + 1], "Nv": [0, -64, 224], "Np": [0, -8, 500], "K": [0, -256, 192, 320],
    }, [
        dict(Nv=1024, Np=520), dict(M=32704),                    # N1 + N2 > 1536; fewer than 128 x 256 rows
        dict(hm_hd=32), dict(hm_rows=100), dict(hm_hd=-8, hm_rows=100), dict(hm_hd=12, hm_rows=100),
        dict(hm_hd=48, hm_rows=100), dict(hm_hd=32, hm_rows=300), dict(hm_hd=32, hm_rows=-100),
        dict(x=BAD, M=I31 + 1), dict(x=BAD, K=192), dict(x=BAD, hm_hd=12, hm_rows=100), dict(hm_hd=12, hm_rows=100, K=192),
    ])


def split_rows():
    order = ("stream", "x", "pos", "w", "bias", "mask", "value", "packed", "M", "Nv", "Np", "K", "hm_rows", "hm_hd")
    base = dict(stream=NULL, x=P, pos=P, w=P, bias=NULL, mask=NULL, value=P, packed=P, M=40000, Nv=256, Np=512, K=256,
                hm_rows=0, hm_hd=0)
    cases = [_vary(base, **c) for c in split_cases("pos") + [dict(pos=NULL), dict(pos=NULL, x=NULL), dict(pos=NULL, K=192)]]
    return [["codetr_encoder_projections_*", [c[k] for k in order]] for c in cases]


def posgen_rows():
    order = ("stream", "x") + tuple(f"yc{i}" for i in range(5)) + tuple(f"xc{i}" for i in range(5)) + (
        "shapes", "L", "le", "temperature", "scale", "eps", "offset", "normalize", "w", "bias", "mask", "value", "packed",
        "M", "S", "Nv", "Np", "K", "hm_rows", "hm_hd")
    base = dict(stream=NULL, x=P, yc0=P, yc1=P, yc2=NULL, yc3=NULL, yc4=NULL, xc0=P, xc1=P, xc2=NULL, xc3=NULL, xc4=NULL,
                shapes=[100, 200, 100, 200], L=2, le=P, temperature=10000.0, scale=6.283185, eps=1e-6, offset=0.0,
                normalize=1, w=P, bias=NULL, mask=NULL, value=P, packed=P, M=40000, S=40000, Nv=256, Np=512, K=256,
                hm_rows=0, hm_hd=0)
    six = [10, 10] * 6
    own = [
        dict(shapes=NULL), dict(S=0), dict(S=-40000), dict(L=0), dict(L=-1), dict(temperature=0.0), dict(temperature=-1.0),
        dict(L=6, shapes=six),                                   # more levels than the kernel holds
        dict(L=6, shapes=six, x=NULL), dict(L=6, shapes=six, M=I31 + 1), dict(L=6, shapes=six, x=BAD),
        dict(L=6, shapes=six, K=192), dict(L=6, shapes=six, S=30000),
        dict(S=30000),                                           # M % S
        dict(S=30000, M=I31 + 1), dict(S=30000, x=BAD), dict(S=30000, K=192), dict(S=30000, x=NULL),
        dict(M=40000 * 60000), dict(M=40000 * 60000, x=BAD),     # whole images, too many rows
        dict(M=20000, S=20000, L=1, shapes=[100, 200]),          # fewer than 128 x 256 rows
        dict(yc1=NULL), dict(xc0=NULL),                          # a level without its running sums
        dict(shapes=[1, 40000, 100, 200], M=60000, S=60000), dict(shapes=[100, 200, 40000, 1], M=60000, S=60000),
        dict(shapes=[0, 200, 100, 200]), dict(shapes=[100, 200, 100, -200]),
        dict(shapes=[100, 200, 100, 100]), dict(shapes=[100, 200, 100, 300]),   # the levels do not add up to S
        dict(shapes=[100, 200, 100, 100], K=192), dict(shapes=[100, 200, 100, 100], yc1=NULL),
    ]
    cases = [_vary(base, **c) for c in split_cases("le") + own]
    return [["codetr_encoder_projections_posgen_*", [c[k] for k in order]] for c in cases]


def main():
    lib = bind(sys.argv[1])
    rows = []
    for entry, args in (linear_rows() + f16out_rows() + xadd_rows() + ln_rows() + splitk_rows() + conv_rows() + split_rows()
                        + posgen_rows()):
        codes = {call(lib, name, args) for name in entries(entry)}
        assert len(codes) == 1, f"{entry}{tuple(args)}: the element types disagree, {codes}"
        rc = codes.pop()
        assert rc < 0, f"{entry}{tuple(args)} is accepted ({rc}): a launch has no place in this table"
        rows.append([entry, args, rc])
    with open(OUT, "w") as f:
        f.write('{"rows": [\n' + ",\n".join(json.dumps(r) for r in rows) + '\n],\n"queries": ' + json.dumps(queries(lib))
                + "}\n")
    codes = sorted({r[2] for r in rows})
    print(f"wrote {OUT}: {len(rows)} rows, codes {codes}, {os.path.getsize(OUT) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
