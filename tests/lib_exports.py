"""What a built library exports: the one reader of ``nm`` for the tests that compare export tables with ``PROTOTYPES``."""
import subprocess


def exports(path):
    """The defined dynamic function symbols of the shared library ``path``, without the linker's own (``_init``, ``_fini``, ``__*``)."""
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if len(ln.split()) >= 3 and ln.split()[-2] in "TtWw"}
    return {n for n in exported if not n.startswith(("_init", "_fini", "__"))}
