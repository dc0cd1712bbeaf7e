"""The vector of every application whose state is one or two planes of grid values: one definition of the arithmetic, the norm, the
clones and the accessors. A vector class is a declaration: its docstring, its base (OnePlaneVector ``(nx, ny)``, TwoPlaneVector ``(nx)``)
and, where its clone() has always copied the array, CLONE_COPIES."""
import numpy as np

from pymgrit_amd.core.vector import Vector


class PlaneVector(Vector):
    """the 2-norm over all values; _args(): the constructor's arguments, _shape(): the shape of the values. CLONE_COPIES: clone()
    copies the array -- the classes differ in this, and each keeps what it did"""
    CLONE_COPIES = False

    def _like(self, values):
        out = type(self)(*self._args())
        out.set_values(values)
        return out

    def __add__(self, other):
        return self._like(self.get_values() + other.get_values())

    def __sub__(self, other):
        return self._like(self.get_values() - other.get_values())

    def __mul__(self, other):
        return self._like(self.get_values() * other)

    def norm(self):
        return np.linalg.norm(self.values)

    def clone(self):
        return self._like(self.get_values().copy() if self.CLONE_COPIES else self.get_values())

    def clone_zero(self):
        return type(self)(*self._args())

    def clone_rand(self):
        return self._like(np.random.rand(*self._shape()))

    def set_values(self, values):
        self.values = values

    def get_values(self):
        return self.values

    def pack(self):
        return self.values

    def unpack(self, values):
        self.values = values


class OnePlaneVector(PlaneVector):
    def __init__(self, nx, ny):
        super().__init__()
        self.nx = nx
        self.ny = ny
        self.values = np.zeros((nx, ny))

    def _args(self):
        return self.nx, self.ny

    _shape = _args


class TwoPlaneVector(PlaneVector):
    def __init__(self, nx):
        super().__init__()
        self.nx = nx
        self.values = np.zeros((2, nx, nx))

    def _args(self):
        return (self.nx,)

    def _shape(self):
        return 2, self.nx, self.nx
