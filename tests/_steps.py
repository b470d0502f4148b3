"""`run_sample.main` as the step tests call it: whatever the run does, the log file it put in place of stdout is closed, stdout
is the caller's again and the worker processes are gone."""
import sys


def run_sample_main(argv, shutdown=True):
    """-> run_sample.main(argv).  `shutdown=False` leaves the worker pool alive for the caller's next run."""
    import run_sample
    from irn_amd.misc import pyutils
    from irn_amd.step import _common
    stdout = sys.stdout
    try:
        return run_sample.main(argv)
    finally:
        if isinstance(sys.stdout, pyutils.Logger):
            sys.stdout.close()
        sys.stdout = stdout
        if shutdown:
            _common.shutdown_workers()
