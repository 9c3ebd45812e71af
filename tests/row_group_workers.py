"""Worker functions of the tests of the row families per peer group (importable by spawned processes): the small exact window
of tests/row_group_oracle_backend.py with its four logical ranks spread over ``world`` processes.  ``cpu=True`` installs the
checker backend with the grouped methods as its first statement (``mp_util.run_ranks`` installs the plain one); otherwise the
active backend is the product's."""
import row_group_oracle_backend as rg

KERNELS = ("beat", "stretch")


def window_reports(rank, world, reports=2, cpu=False, peer_groups="block:2", gather_on_rank0=True, **options):
    """``reports`` windows (the general report, then planned ones); per report the four families' dicts, or None where this
    rank holds no report, and -- on the checker -- the grouped calls this rank's backend saw."""
    from nvrx_straggler import backend

    if cpu:
        backend.set_backend(rg.RowGroupOracleBackend())
    be = backend.get_backend()
    local = rg.LOCAL_RANKS // world
    gen, rings, rows = rg.make(be, KERNELS, peer_groups=peer_groups, local_ranks=local, gather_on_rank0=gather_on_rank0,
                               **options)
    try:
        out = []
        for window in range(reports):
            rep = rg.report(gen, rings, rows, KERNELS, window, local_ranks=local, first_rank=rank * local)
            out.append(None if rep is None else rg.family_scores(rep))
        return {"reports": out, "grouped_calls": list(getattr(be, "row_group_calls", ()))}
    finally:
        gen.close()
        rings.close()
