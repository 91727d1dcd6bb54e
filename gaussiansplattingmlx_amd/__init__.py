from .features import FeatureField  # noqa: F401
