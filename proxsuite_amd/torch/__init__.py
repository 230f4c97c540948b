"""`proxsuite.torch` of the reference: the QPLayer forward on the MI355X batch solver."""
from .qplayer import QPFunction, QPFunctionBox, solution_jacobians

__all__ = ["QPFunction", "QPFunctionBox", "solution_jacobians"]
