"""Drop-in for the part of InsightFace (0.7.3) the reference pipelines use: insightface.app.FaceAnalysis with its detector
(SCRFD, model_zoo/retinaface.py RetinaFace) running on the GPU through libffp (ffp_scrfd_*). The landmark, gender/age and
recognition models of a pack are not run."""
__version__ = "0.7.3"
