"""Helpers of the tests that ask the GEMM launch plans (mmdti_gemm_plan / mmdti_linear_dw_grouped_plan): build the argument list of a
call from a short description, and read the plan back in a comparable form.  No GPU needed: pointers are fake, aligned addresses."""
import ctypes

ACT_NONE, ACT_GELU, ACT_GELU_BWD, ACT_GELU_G, ACT_MUL_AUX = 0, 1, 2, 4, 5
FAMILY = ["gemm_bf16_kernel", "gemm_glds_kernel", "gemm_glds_kernel", "gemm_glds_kernel", "gemm_glds_tall_kernel", "gemm_small_kernel",
          "gemm_big_kernel"]
PTR = 0x10000          # fake, 16-byte aligned device addresses: the queries never dereference them


def r8(n):
    return (n + 7) // 8 * 8


def case(M, N, K, tA=0, tB=0, sk=1, out="bf16", ab16=0, bcvt=0, batch=(1, 1), bias=0, residual=0, act=ACT_NONE, aux_in=0, aux_out=0,
         colsum=0, arowsum=0, ws=0, beta=0.0, alpha=1.0, ldc=None, lda=None, ldb=None):
    return dict(M=M, N=N, K=K, tA=tA, tB=tB, sk=sk, out=out, ab16=ab16, bcvt=bcvt, batch=batch, bias=bias, residual=residual, act=act,
                aux_in=aux_in, aux_out=aux_out, colsum=colsum, arowsum=arowsum, ws=ws, beta=beta, alpha=alpha, ldc=ldc, lda=lda, ldb=ldb)


def gemm_call_args(c):
    """The argument list of mmdti_gemm_bf16 without the stream, as ops.gemm builds it (natural leading dimensions)."""
    M, N, K = c["M"], c["N"], c["K"]
    lda = c["lda"] or (r8(M) if c["tA"] else r8(K))
    ldb = c["ldb"] or (r8(N) if c["tB"] else r8(K))
    ldc = c["ldc"] or N
    dt = {"f32": 0, "bf16": 1, "atomic": 2, "f16": 3}[c["out"]] | (16 if c["ab16"] else 0) | (32 if c["bcvt"] else 0)
    bo, bi = c["batch"]
    sA = (bi * M * lda, M * lda) if bo * bi > 1 else (0, 0)
    sB = (bi * N * ldb, N * ldb) if bo * bi > 1 else (0, 0)
    sC = (bi * M * ldc, M * ldc) if bo * bi > 1 else (0, 0)
    p = lambda on: PTR if on else 0
    return [PTR, PTR, PTR, M, N, K, lda, ldb, ldc, c["tA"], c["tB"], bo, bi, sA[0], sA[1], sB[0], sB[1], sC[0], sC[1], c["sk"],
            c["alpha"], c["beta"], p(c["bias"]), p(c["residual"]), ldc, c["act"], p(c["aux_in"]), p(c["aux_out"]), N, dt, 0.0, 0, 0,
            p(c["colsum"]), p(c["arowsum"]), p(c["ws"]), c["ws"]]


def kernel_name(p):
    """the instance a plan names, spelled as the symbol demangles (every template argument, defaults included)"""
    fam, ta, tb, fast, f16, bcvt = p[:6]
    b = lambda v: "true" if v else "false"
    if fam == 0:
        targs = [b(ta), b(tb), b(fast), b(f16), b(bcvt)]
    elif fam in (1, 2, 3):
        targs = [b(ta), b(tb), str(fam - 1), b(f16), b(bcvt)]
    elif fam in (4, 5):
        targs = [b(tb), b(f16)]
    else:
        targs = [b(ta), b(tb), b(f16), b(bcvt), "false"]            # (no mmdti_gemm_bf16 shape takes a TAIL instance)
    return f"{FAMILY[fam]}<{', '.join(targs)}>"


def plan_of(lib, c):
    out = (ctypes.c_int * 15)()
    lib.mmdti_gemm_plan(*gemm_call_args(c), out)
    p = list(out)
    # (kernel, grid x, grid z, block, LDS, splitk, mstep, slabs, stream_c, arowsum)
    return (kernel_name(p), p[6], p[7], p[8], p[9], p[10], p[11], p[12], p[13], p[14])


def grouped_plan(lib, shapes, rows, x_f16=0):
    """mmdti_linear_dw_grouped's plan for problems [(n_out, n_in)] over `rows` tokens ->
    ((kernel, grid x, grid z, block, LDS, splits, atomic, second pass), workspace bytes demanded)"""
    n = len(shapes)
    out, ws = (ctypes.c_int * 9)(), ctypes.c_longlong()
    lib.mmdti_linear_dw_grouped_plan(n, (ctypes.c_int * n)(*[s[0] for s in shapes]), (ctypes.c_int * n)(*[s[1] for s in shapes]), rows, x_f16, out,
                                     ctypes.byref(ws))
    small, gx, gz, block, lds, sk, ktail, atomic, bcvt = list(out)
    b = lambda v: "true" if v else "false"
    name = f"gemm_small_dw_grouped_kernel<3, {b(bcvt)}>" if small else f"gemm_big_grouped_kernel<{b(bcvt)}, {b(ktail)}>"
    return (name, gx, gz, block, lds, sk, atomic, int(not small and not atomic)), ws.value


def dw_case(ops, n_out, n_in, rows, db, x_f16=0):
    """the call ops.linear_bwd_weight makes for dw [n_out, n_in] over `rows` tokens"""
    return case(n_out, n_in, rows, tA=1, tB=1, sk=ops._splitk_for(n_out, n_in, rows), out="atomic", arowsum=int(db), bcvt=x_f16,
                ws=4 * ops.dw_workspace_floats(n_out, n_in, rows))
