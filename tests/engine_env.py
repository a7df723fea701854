"""Engines under environment switches, for the tests that compare a switched path with the
shipped one."""
import contextlib
import os


@contextlib.contextmanager
def engine_env(env, probes=False):
    """A second Engine(0) created with the environment switches `env` set -- a context reads them
    when it is created --, the environment restored at once; the engine is closed on exit.
    probes: on the probe library."""
    from bayesian_quadrature_amd import Engine
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = Engine(0, probes=probes)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        yield eng
    finally:
        eng.close()
