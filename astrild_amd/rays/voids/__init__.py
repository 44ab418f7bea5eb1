from .tunnel import TunnelsFinder, TunnelsFinderWarning  # noqa: F401
from .watershed import WatershedFinder, WatershedFinderWarning  # noqa: F401
