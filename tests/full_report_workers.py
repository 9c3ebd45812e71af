"""Worker functions of the all-options tests (importable by spawned processes): the job of tests/full_report_script.py with
its eight logical ranks spread over ``world`` processes.  ``cpu=True`` installs the composed checker backend as its first
statement (``mp_util.run_ranks`` installs the plain one); otherwise the active backend is the product's."""
import full_report_script as fs


def composed_reports(rank, world, gather_on_rank0=True, cpu=False, emulate_fused=False, asynchronous=False, windows=3,
                     features=None, **options):
    """``windows`` composed reports (the general report, then planned ones), every report read only after the last was
    issued; per report what ``fs.read`` and ``fs.identified`` say, or None where this rank holds no report, and -- on the
    checker -- this rank's call counters and the ``first_rank`` its grouped steps were given."""
    from nvrx_straggler import backend

    if cpu:
        from full_oracle_backend import FullOracleBackend

        backend.set_backend(FullOracleBackend(emulate_fused=emulate_fused))
    be = backend.get_backend()
    local = fs.RANKS // world
    job = fs.Job(be, features, local_ranks=local, first_rank=rank * local, gather_on_rank0=gather_on_rank0,
                 asynchronous=asynchronous, **options)
    try:
        held = [job.report(w) for w in range(windows)]
        out = [None if rep is None else {"read": fs.read(rep, features), "identified": fs.identified(rep, features)}
               for rep in held]
        counters = {k: v for k, v in vars(be).items() if k.endswith("_calls")} if cpu else {}
        first = sorted({a[5] for a in getattr(be, "row_group_args", ())} | {a[5] for a in getattr(be, "slack_group_args", ())})
        return {"reports": out, "counters": counters, "first_ranks": first}
    finally:
        job.close()
