// Mirrors Runtime/RHI/DebugContext.{h,cpp}: the line list everything the engine shows for debugging is built from -- DrawLine (:76-98) and the shapes over it
// (DrawAABB :100-116, DrawArrow :118-127, DrawOrigin :129-138, DrawFrustum :140-158, DrawSphere :17-63) in the reference's segment order and fp32 arithmetic --,
// Tick (:259-314) with its RemoveAtSwap lifetime bookkeeping, the vertex / index upload (UpdateDebugMesh :316-380) and DrawDebugMesh (:382-398), the one draw
// the DebugDraw node replays.  glm types are plain float arrays here (a mat4 is 16 floats, column-major).  Not mirrored: DrawPlane (two equal segments from a
// normalised Math::Plane), DrawLightCascades (needs LightingECS's cascade levels and glm::inverse; it is DrawFrustum and DrawLine over corners the caller can
// compute), DrawCone (empty in the reference).
#pragma once
#include "Types.h"

namespace Sailor::RHI {

using VertexP3C4 = SailorVertexP3C4; // RHI/Types.h VertexP3C4: m_position, m_color

class DebugContext {
public:
    void DrawLine(const float* start, const float* end, const float* color, float duration = 0.0f);
    void DrawAABB(const float* aabbMin, const float* aabbMax, const float* color, float duration = 0.0f);
    void DrawArrow(const float* start, const float* end, const float* color, float duration = 0.0f);
    void DrawOrigin(const float* position, const float* origin, float size = 1.0f, float duration = 0.0f);
    void DrawSphere(const float* position, float radius, const float* color, float duration = 0.0f);
    void DrawFrustum(const float* corners /* Frustum::GetCorners(): 8 x 3 */, const float* color, float duration = 0.0f);

    // :259-314.  m_numRenderedVertices is set BEFORE the lifetimes run down: a line that expires in this tick is still drawn in the frame of this tick, from
    // the buffer uploaded here.  As in the reference, a tick that finds no lines returns at once and leaves m_numRenderedVertices as it was.
    void Tick(RHICommandListPtr transferCmd, float deltaTime);
    // :382-398: BindMaterial, BindVertexBuffer, BindIndexBuffer, PushConstants(viewProjection), DrawIndexed(m_numRenderedVertices, 1, 0, 0, 0); nothing when
    // there is nothing to draw.  (SetDefaultViewport has no counterpart: a pass covers its attachments here.)
    void DrawDebugMesh(RHICommandListPtr secondaryDrawCmdList, const float* viewProjection) const;

    // the bookkeeping half of Tick, without a driver (:291-313): run the lifetimes down, RemoveAtSwap what expired, remember where the buffer changed
    void ExpireLines(float deltaTime);
    // the index half of UpdateDebugMesh (:326-336): index i = i, grown on demand; true if it grew
    bool GrowIndices();

    const TVector<VertexP3C4>& GetLineVertices() const { return m_lineVertices; }
    const TVector<float>& GetLifetimes() const { return m_lifetimes; }
    const TVector<uint32_t>& GetCachedIndices() const { return m_cachedIndices; }
    uint32_t GetNumRenderedVertices() const { return m_numRenderedVertices; }
    int32_t GetLineVerticesOffset() const { return m_lineVerticesOffset; }
    void Clear();

protected:
    void UpdateDebugMesh(RHICommandListPtr transferCmdList);

    struct { RHIBufferPtr m_vertexBuffer, m_indexBuffer; bool IsReady() const { return m_vertexBuffer && m_indexBuffer; } } m_cachedMesh; // RHI/Mesh.h, as far as used
    bool m_bHasMesh = false;
    RHIMaterialPtr m_material;
    TVector<uint32_t> m_cachedIndices;
    TVector<VertexP3C4> m_lineVertices;
    TVector<float> m_lifetimes;
    int32_t m_lineVerticesOffset = -1;
    uint32_t m_numRenderedVertices = 0;
    bool m_bShouldUpdateMeshThisFrame = false;
};

} // namespace Sailor::RHI
