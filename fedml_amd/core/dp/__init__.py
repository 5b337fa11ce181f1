"""Differential privacy (reference: python/fedml/core/dp)."""
from .fedml_differential_privacy import FedMLDifferentialPrivacy  # noqa: F401
