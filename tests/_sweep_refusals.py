"""Every PG_EINVAL of pg_refine_sweep, pg_refine_sweep_totals and pg_refine_sweep_plan, by the name of the argument.  The checks
come before any HIP call, so the pointers below are never dereferenced: the same function runs with no GPU
(tests/test_refiner_fit_cpu.py) and on one (tests/test_gpu_refine_sweep.py)."""
import ctypes as C

PG_EINVAL = -1
FAKE = C.c_void_p(0x1000)          # a non-null pointer that no refused call may touch
NULL = C.c_void_p(0)


def refused(L, rc, *names):
    msg = (L.pg_last_error() or b"").decode()
    assert rc != 0, f"accepted; expected a refusal naming {names}"
    assert all(n in msg for n in names), f"the refusal {msg!r} does not name {names}"


def check_refusals(L):
    einval = PG_EINVAL

    def sweep(SC=4, B=8, n_eval=5, cand_prob=FAKE, k=5, topks=(1, 5), temps=(0.5, 1.0), max_kms=(10.0, float("inf")), nK=None, nT=None,
              nR=None, scratch=FAKE, init=FAKE, choice=FAKE):
        ka = None if topks is None else (C.c_int32 * max(len(topks), 1))(*topks)
        ta = None if temps is None else (C.c_float * max(len(temps), 1))(*temps)
        ra = None if max_kms is None else (C.c_double * max(len(max_kms), 1))(*max_kms)
        return L.pg_refine_sweep(scratch, SC, B, n_eval, cand_prob, k, init, ka, len(topks or ()) if nK is None else nK, ta,
                                 len(temps or ()) if nT is None else nT, ra, len(max_kms or ()) if nR is None else nR, choice, NULL, NULL)

    for rc, names in ((lambda: sweep(SC=8), ("SC",)), (lambda: sweep(B=-1), ("B",)), (lambda: sweep(n_eval=0), ("n_eval",)), (lambda: sweep(n_eval=65, k=65), ("n_eval",)),
                      (lambda: sweep(nK=0), ("nK",)), (lambda: sweep(nT=0), ("nT",)), (lambda: sweep(nR=0), ("nR",)),
                      (lambda: sweep(n_eval=5, k=4), ("n_eval", "k")),
                      (lambda: sweep(topks=(1, 0)), ("topks[1]",)), (lambda: sweep(topks=(6,)), ("topks[0]",)),
                      (lambda: sweep(temps=(1.0, 0.0)), ("temps[1]",)), (lambda: sweep(temps=(-1.0,)), ("temps[0]",)),
                      (lambda: sweep(temps=(float("inf"),)), ("temps[0]",)), (lambda: sweep(temps=(float("nan"),)), ("temps[0]",)),
                      (lambda: sweep(max_kms=(1.0, float("nan"))), ("max_kms[1]",)),
                      (lambda: sweep(topks=None, nK=1), ("topks",)), (lambda: sweep(temps=None, nT=1), ("temps",)), (lambda: sweep(max_kms=None, nR=1), ("max_kms",)),
                      (lambda: sweep(scratch=NULL), ("scratch",)), (lambda: sweep(init=NULL), ("init_llh",)), (lambda: sweep(choice=NULL), ("choice",))):
        rc = rc()
        assert rc == einval
        refused(L, rc, *names)
    # G = nK * nT * nR above 2^20
    big = tuple([1] * 1025)
    rc = sweep(topks=big, temps=tuple([1.0] * 1024), max_kms=(1.0, 2.0))
    assert rc == einval
    refused(L, rc, "G")
    # an empty batch is a no-op, with null buffers
    assert sweep(B=0, scratch=NULL, init=NULL, choice=NULL, cand_prob=NULL, k=0) == 0
    # cand_prob NULL: k is not looked at
    rc = sweep(cand_prob=NULL, k=0, topks=(9,))
    assert rc == einval
    refused(L, rc, "topks[0]")

    def tot(G=4, B=8, n_eval=5, V=3, choice=FAKE, values=FAKE, out=FAKE):
        return L.pg_refine_sweep_totals(choice, G, B, n_eval, values, V, out, NULL)

    for rc, names in ((lambda: tot(G=0), ("G",)), (lambda: tot(G=(1 << 20) + 1), ("G",)), (lambda: tot(B=-1), ("B",)), (lambda: tot(n_eval=0), ("n_eval",)),
                      (lambda: tot(n_eval=65), ("n_eval",)), (lambda: tot(V=0), ("V",)), (lambda: tot(V=17), ("V",)), (lambda: tot(choice=NULL), ("choice",)),
                      (lambda: tot(values=NULL), ("values",)), (lambda: tot(out=NULL), ("totals",))):
        rc = rc()
        assert rc == einval
        refused(L, rc, *names)

    o = (C.c_int64 * 4)()
    for rc, names in ((lambda: L.pg_refine_sweep_plan(-1, 5, 4, 3, o), ("B",)), (lambda: L.pg_refine_sweep_plan(8, 65, 4, 3, o), ("n_eval",)),
                      (lambda: L.pg_refine_sweep_plan(8, 5, 0, 3, o), ("G",)), (lambda: L.pg_refine_sweep_plan(8, 5, 4, 17, o), ("V",)),
                      (lambda: L.pg_refine_sweep_plan(8, 5, 4, 3, None), ("out",))):
        rc = rc()
        assert rc == einval
        refused(L, rc, *names)
    assert L.pg_refine_sweep_plan(8192, 50, 64 * 25 * 9, 12, o) == 0
    assert list(o) == [64, 50 * 64 * 13, 128, 64 * 25 * 9 * 8192]
    assert L.pg_refine_sweep_plan(65, 64, 1, 1, o) == 0 and list(o) == [64, 64 * 64 * 13, 2, 65]
