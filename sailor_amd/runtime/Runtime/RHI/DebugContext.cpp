#include "DebugContext.h"
#include "Renderer.h"
#include <algorithm>
#include <cmath>

using namespace Sailor;
using namespace Sailor::RHI;

namespace {
struct V3 { float x, y, z; };
inline V3 v3(const float* p) { return { p[0], p[1], p[2] }; }
inline V3 operator+(V3 a, V3 b) { return { a.x + b.x, a.y + b.y, a.z + b.z }; }
inline V3 operator*(V3 a, float s) { return { a.x * s, a.y * s, a.z * s }; }
const float Pi = 3.1415926f; // Math/Math.h:14
// TVector::RemoveAtSwap (Containers/Vector.h:514-529): the last `count` elements take the removed ones' places, in order
template <typename T> void RemoveAtSwap(TVector<T>& v, size_t index, size_t count)
{
    for (size_t k = 0; k < count; k++) v[index + k] = v[v.size() - count + k];
    v.resize(v.size() - count);
}
} // namespace

void DebugContext::DrawLine(const float* start, const float* end, const float* color, float duration)
{
    VertexP3C4 startVertex, endVertex;
    for (int k = 0; k < 3; k++) { startVertex.position[k] = start[k]; endVertex.position[k] = end[k]; }
    for (int k = 0; k < 4; k++) startVertex.color[k] = endVertex.color[k] = color[k];
    m_lineVertices.push_back(startVertex);
    m_lineVertices.push_back(endVertex);
    m_lifetimes.push_back(duration);
    if (m_lineVerticesOffset == -1) m_lineVerticesOffset = (int32_t)m_lifetimes.size() - 1; // (:92-95, as the reference has it: a line index, not a vertex index)
    m_bShouldUpdateMeshThisFrame = true;
}

void DebugContext::DrawAABB(const float* mn, const float* mx, const float* color, float duration)
{
    auto line = [&](V3 a, V3 b) { DrawLine(&a.x, &b.x, color, duration); };
    const V3 a = v3(mn), b = v3(mx);
    line(a, { b.x, a.y, a.z }); line(a, { a.x, b.y, a.z }); line(a, { a.x, a.y, b.z });
    line(b, { a.x, b.y, b.z }); line(b, { b.x, a.y, b.z }); line(b, { b.x, b.y, a.z });
    line({ a.x, b.y, b.z }, { a.x, b.y, a.z }); line({ a.x, b.y, b.z }, { a.x, a.y, b.z }); line({ a.x, a.y, b.z }, { b.x, a.y, b.z });
    line({ b.x, a.y, b.z }, { b.x, a.y, a.z }); line({ b.x, a.y, a.z }, { b.x, b.y, a.z }); line({ b.x, b.y, a.z }, { a.x, b.y, a.z });
}

void DebugContext::DrawArrow(const float* start, const float* end, const float* color, float duration)
{
    const V3 s = v3(start), e = v3(end), d = { e.x - s.x, e.y - s.y, e.z - s.z };
    const float length = std::sqrt((d.x * d.x + d.y * d.y) + d.z * d.z) * 0.1f; // glm::length: sqrt(dot)
    auto line = [&](V3 a, V3 b) { DrawLine(&a.x, &b.x, color, duration); };
    const V3 up = { 0, 1, 0 }, left = { -1, 0, 0 }, forward = { 0, 0, -1 }; // Math.h:19-25
    line(s, e);
    line(e + up * length, e + (up * -1.0f) * length);
    line(e + left * length, e + (left * -1.0f) * length);
    line(e + forward * length, e + (forward * -1.0f) * length);
}

void DebugContext::DrawOrigin(const float* position, const float* m, float size, float duration)
{
    // glm's mat4 * vec4: (c0 x + c1 y) + (c2 z + c3 w), here with w == 0 and two of x, y, z zero
    auto axis = [&](float x, float y, float z) {
        V3 r;
        float* o = &r.x;
        for (int k = 0; k < 3; k++) o[k] = (m[k] * x + m[4 + k] * y) + (m[8 + k] * z + m[12 + k] * 0.0f);
        return r;
    };
    const V3 p = v3(position), x = p + axis(size, 0, 0), y = p + axis(0, size, 0), z = p + axis(0, 0, size);
    const float red[4] = { 1, 0, 0, 1 }, green[4] = { 0, 1, 0, 1 }, blue[4] = { 0, 0, 1, 1 };
    DrawLine(position, &x.x, red, duration);
    DrawLine(position, &y.x, green, duration);
    DrawLine(position, &z.x, blue, duration);
}

void DebugContext::DrawSphere(const float* position, float radius, const float* color, float duration)
{
    const int32_t SegmentsX = 7, SegmentsY = 7;
    const V3 p = v3(position);
    for (int32_t i = 0; i <= SegmentsX; i++) {
        const float lat0 = Pi * (-0.5f + (float)(i - 1) / SegmentsX), z0 = std::sin(lat0), zr0 = std::cos(lat0);
        const float lat1 = Pi * (-0.5f + (float)i / SegmentsX), z1 = std::sin(lat1), zr1 = std::cos(lat1);
        V3 v1, v2, v3_ = {}, v4 = {};
        bool bContinuation = false;
        for (int32_t j = 0; j <= SegmentsY; j++) {
            const float lng = 2 * Pi * (float)(j - 1) / SegmentsY, x = std::cos(lng), y = std::sin(lng);
            v1 = p + V3 { radius * x * zr0, radius * z0, radius * y * zr0 };
            v2 = p + V3 { radius * x * zr1, radius * z1, radius * y * zr1 };
            if (!bContinuation) bContinuation = true;
            else { DrawLine(&v1.x, &v3_.x, color, duration); DrawLine(&v2.x, &v4.x, color, duration); }
            DrawLine(&v1.x, &v2.x, color, duration);
            v3_ = v1; v4 = v2;
        }
    }
}

void DebugContext::DrawFrustum(const float* c, const float* color, float duration)
{
    const float white[4] = { 1, 1, 1, 1 };
    auto line = [&](int a, int b, const float* col) { DrawLine(c + 3 * a, c + 3 * b, col, duration); };
    line(4, 5, color); line(5, 6, color); line(6, 7, color); line(7, 4, color);
    line(0, 1, white); line(1, 2, white); line(2, 3, white); line(3, 0, white);
    line(4, 0, color); line(5, 1, color); line(6, 2, color); line(7, 3, color);
}

void DebugContext::ExpireLines(float deltaTime)
{
    m_lineVerticesOffset = -1;
    for (uint32_t i = 0; i < m_lifetimes.size(); i++) {
        m_lifetimes[i] -= deltaTime;
        if (m_lifetimes[i] < 0.0f) {
            RemoveAtSwap(m_lifetimes, i, 1);
            RemoveAtSwap(m_lineVertices, (size_t)i * 2, 2);
            if (m_lineVerticesOffset == -1) m_lineVerticesOffset = (int32_t)(i * 2);
            i--; // (wraps at i == 0 and comes back with the increment, as in the reference)
        }
    }
    if (m_lineVerticesOffset == (int32_t)m_lineVertices.size()) m_lineVerticesOffset = -1;
}

bool DebugContext::GrowIndices()
{
    if (m_cachedIndices.size() >= m_lineVertices.size()) return false;
    const uint32_t start = (uint32_t)m_cachedIndices.size();
    m_cachedIndices.resize(m_lineVertices.size());
    for (uint32_t i = start; i < m_lineVertices.size(); i++) m_cachedIndices[i] = i;
    return true;
}

void DebugContext::Tick(RHICommandListPtr transferCmd, float deltaTime)
{
    if (m_lineVertices.empty()) return;
    auto driver = Renderer::GetDriver();
    if (!m_material) { // :270-285: RenderState(depth test, depth write, no bias, ..., ECullMode::Back, EBlendMode::None, EFillMode::Line), LineList
        auto pShader = driver->CreateShader("Shaders/Gizmo.shader");
        if (!pShader || !pShader->IsReady()) return; // LoadShader_Immediate failed
        m_bHasMesh = true; // m_cachedMesh = renderer->CreateMesh()
        m_material = driver->CreateMaterial(pShader);
        m_material->m_topology = EPrimitiveTopology::LineList;
    }
    UpdateDebugMesh(transferCmd);
    m_numRenderedVertices = (uint32_t)m_lineVertices.size();
    ExpireLines(deltaTime);
}

void DebugContext::UpdateDebugMesh(RHICommandListPtr transferCmdList)
{
    if (m_lineVertices.empty()) return;
    auto driver = Renderer::GetDriver();
    auto commands = Renderer::GetDriverCommands();
    const bool bNeedUpdateIndexBuffer = GrowIndices();
    const size_t bufferSize = sizeof(VertexP3C4) * m_lineVertices.size(), indexBufferSize = sizeof(uint32_t) * m_lineVertices.size();
    const bool bShouldCreateVertexBuffer = !m_cachedMesh.m_vertexBuffer || m_cachedMesh.m_vertexBuffer->m_size < bufferSize;
    const bool bNeedUpdateVertexBuffer = m_lineVerticesOffset != -1 || bShouldCreateVertexBuffer || m_bShouldUpdateMeshThisFrame;
    if (bNeedUpdateVertexBuffer || bNeedUpdateIndexBuffer) {
        if (bShouldCreateVertexBuffer) { // CreateBuffer(cmd, data, size, VertexBuffer_Bit): here an allocation and an upload
            m_cachedMesh.m_vertexBuffer = driver->CreateBuffer(bufferSize);
            if (m_cachedMesh.m_vertexBuffer) commands->UpdateBuffer(transferCmdList, m_cachedMesh.m_vertexBuffer, m_lineVertices.data(), bufferSize, 0);
        } else {
            // (:355, as the reference has it: the offset DrawLine left is a line index, the one ExpireLines left a vertex index; either is at or before the
            // first vertex that changed and never past the end, and everything from there on is uploaded)
            m_lineVerticesOffset = std::max(m_lineVerticesOffset, 0);
            commands->UpdateBuffer(transferCmdList, m_cachedMesh.m_vertexBuffer, m_lineVertices.data() + m_lineVerticesOffset,
                                   bufferSize - sizeof(VertexP3C4) * m_lineVerticesOffset, sizeof(VertexP3C4) * m_lineVerticesOffset);
        }
        if (bNeedUpdateIndexBuffer) {
            if (!m_cachedMesh.m_indexBuffer || m_cachedMesh.m_indexBuffer->m_size < indexBufferSize) {
                m_cachedMesh.m_indexBuffer = driver->CreateBuffer(indexBufferSize);
                if (m_cachedMesh.m_indexBuffer) commands->UpdateBuffer(transferCmdList, m_cachedMesh.m_indexBuffer, m_cachedIndices.data(), indexBufferSize, 0);
            } else
                commands->UpdateBuffer(transferCmdList, m_cachedMesh.m_indexBuffer, m_cachedIndices.data(), indexBufferSize, 0);
        }
    }
    m_bShouldUpdateMeshThisFrame = false;
}

void DebugContext::DrawDebugMesh(RHICommandListPtr secondaryDrawCmdList, const float* viewProjection) const
{
    if (m_numRenderedVertices == 0 || !m_bHasMesh || !m_cachedMesh.IsReady()) return;
    auto commands = Renderer::GetDriverCommands();
    commands->BindMaterial(secondaryDrawCmdList, m_material);
    commands->BindVertexBuffer(secondaryDrawCmdList, m_cachedMesh.m_vertexBuffer, 0);
    commands->BindIndexBuffer(secondaryDrawCmdList, m_cachedMesh.m_indexBuffer, 0);
    commands->PushConstants(secondaryDrawCmdList, m_material, 64, viewProjection);
    commands->DrawIndexed(secondaryDrawCmdList, m_numRenderedVertices, 1, 0, 0, 0);
}

void DebugContext::Clear()
{
    m_cachedMesh.m_vertexBuffer.Clear(); m_cachedMesh.m_indexBuffer.Clear();
    m_material.Clear();
    m_bHasMesh = false;
    m_cachedIndices.clear(); m_lineVertices.clear(); m_lifetimes.clear();
    m_lineVerticesOffset = -1; m_numRenderedVertices = 0; m_bShouldUpdateMeshThisFrame = false;
}
