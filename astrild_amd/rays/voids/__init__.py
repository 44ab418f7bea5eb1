from .tunnel import TunnelsFinder, TunnelsFinderWarning  # noqa: F401
