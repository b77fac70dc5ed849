"""MI355X-native online TSDF fusion + semantics engine (per-frame hot path only).

Drop-in counterparts of the reference's ``modules/pipeline.py`` Pipeline and
``modules/database.py`` Database, backed by hand-written gfx950 HIP kernels behind the
C ABI declared in ``include/ojf.h``.  Beside them: ``render``, ``tracking``, ``projective``, ``color``,
``label_probs``, ``rasterize`` and ``resample`` (re-box, resample and merge fused scenes; ``Database.resample`` /
``recentre`` / ``merge``), ``registration`` (the rigid transform between two fused scenes; ``Database.register``) and
``frames`` (the live depth frame made ready: edge rejection, bilateral filter, normals; ``filter=`` on ``Database``).
"""
__version__ = '0.1.0'
